// Heads + PPO loss + head backward of the teacher update (models_split.py:222-250; frozen_ppo.py:543-570, 618): one set
// of formulas (section 1), three kernels that differ only in how the values reach the lanes (sections 2 - 4), and the
// host function that picks one (section 5).  Included by teacher.h, behind its plan and block reduction helpers.
#pragma once

namespace igi {

struct LossArgs {
  const float* h;        // [2][mb][ldh] last hidden (actor, critic); shared trunk: [mb][ldh]
  float* dh;             // [2][mb][ldh] d(pre-activation) of the last hidden layer; shared trunk: [mb][ldh]
  long long net_stride;  // mb*ldh; shared trunk: 0 (both heads read the one row)
  int shared;            // 1: shared actor-critic trunk (cfg.shared_parameters) -- ONE dZ row, the sum of the heads' shares
  int ldh, H;
  int ld_dh;             // layout of dh (may be the interleaved [row][net][u0p] form)
  long long net_stride_dh;
  const float* Wmu; const float* bmu; const float* Wv; const float* bv; const float* logstd;
  const float* actions; const float* neglogpacs;                  // rollout (time-major)
  const float* adv; const float* values_n; const float* returns_n;  // prepared
  float* mus_w; float* sigmas_w;
  const int64_t* perm;
  long long start;
  int mb, N, T, act, rows_per_wave;
  float e_clip, critic_coef, entropy_coef, bounds_coef;
  double* loss_part;  // [blocks][8]: a_loss, c_loss, bounds, entropy, kl, approx_kl sums; two spare
  const int32_t* stop;  // KL early stopping: the stop word (>= 0: an earlier step of this update stopped it -> no
                        // update_mu_sigma write-back); NULL = off, and for step 0, which no step precedes
  float* head_slab;   // [blocks][head_count]
  int head_count;
};

constexpr float LOG_SQRT_2PI_F = 0.918938533204672741780329736406f;

// ---------------------------------------------------------------------------------------------
// 1. The arithmetic, once.  Plain values in and out: no lane, row or LDS layout in here.  The library is built with
//    -ffp-contract=off, so every expression below rounds as written; the three kernels are bitwise interchangeable
//    up to the order of their head dot products.
// ---------------------------------------------------------------------------------------------
struct ActionConsts { float sig, logsc, var; };
__device__ __forceinline__ ActionConsts action_consts(float logstd) {
  ActionConsts c;
  c.sig = expf(logstd);
  c.logsc = logf(c.sig);  // Normal.log_prob uses scale.log() (torch/distributions/normal.py)
  c.var = c.sig * c.sig;
  return c;
}

// one action dimension of one sample: its terms of neglogp, entropy, bounds loss and KL (each summed over the actions
// by the caller), and what d_mu / d_sigma need again
struct ActionTerms {
  float x, bh, blo;
  float nlp, ent, bl, kl;
  // a lane that owns no action of a live row adds nothing to the sums over the actions
  __device__ __forceinline__ void keep_if(bool on) {
    if (!on) { nlp = 0.f; ent = 0.f; bl = 0.f; kl = 0.f; }
  }
};
__device__ __forceinline__ ActionTerms action_terms(float ac, float mu, float omu, float osig, const ActionConsts& c) {
  ActionTerms t;
  t.x = ac - mu;
  t.bh = fminf(mu - 1.1f, 0.f), t.blo = fminf(-mu + 1.1f, 0.f);
  const float dm = omu - mu;
  t.nlp = (t.x * t.x) / (2.0f * c.var) + c.logsc + LOG_SQRT_2PI_F;
  t.ent = 0.5f + LOG_SQRT_2PI_F + c.logsc;
  t.bl = t.blo * t.blo + t.bh * t.bh;
  // policy_kl(new, old) frozen_ppo.py:854-860
  t.kl = (logf(osig / c.sig + 1e-5f) + (c.var + dm * dm) / (2.0f * (osig * osig + 1e-5f))) - 0.5f;
  return t;
}

// the bounds term as the statistics report it (frozen_ppo.py:554-560): without a positive coefficient b_loss is 0, not the
// sum the coefficient would have multiplied
__device__ __forceinline__ float bounds_stat(float bl, float bounds_coef) { return bounds_coef > 0.f ? bl : 0.f; }

// actor loss (frozen_ppo.py:544-547): the clipped surrogate and d(loss)/d(neglogp), with the mean of the two branches'
// sub-gradients where they tie (torch.max's backward)
struct ActorLoss { float loss, dnlp; };
__device__ __forceinline__ ActorLoss actor_loss(float adv, float old_nlp, float nlp, float lo, float hi) {
  const float ratio = expf(old_nlp - nlp);
  const float rc = fminf(fmaxf(ratio, lo), hi);
  const float s1 = -(adv * ratio), s2 = -(adv * rc);
  const float d1 = adv * ratio;  // d s1 / d nlp
  const float d2 = (ratio >= lo && ratio <= hi) ? d1 : 0.f;
  return {fmaxf(s1, s2), (s1 > s2) ? d1 : ((s1 < s2) ? d2 : 0.5f * (d1 + d2))};
}

// critic loss (frozen_ppo.py:549-552): the clipped value loss and d(loss)/d(value), same tie rule
struct CriticLoss { float loss, dv; };
__device__ __forceinline__ CriticLoss critic_loss(float v, float R, float vp, float e_clip) {
  const float dvp = v - vp;
  const float vclip = vp + fminf(fmaxf(dvp, -e_clip), e_clip);
  const float l1 = (v - R) * (v - R), l2 = (vclip - R) * (vclip - R);
  const float g1 = 2.0f * (v - R);
  const float g2 = (dvp >= -e_clip && dvp <= e_clip) ? 2.0f * (vclip - R) : 0.f;
  return {fmaxf(l1, l2), (l1 > l2) ? g1 : ((l1 < l2) ? g2 : 0.5f * (g1 + g2))};
}

// the KL estimator of frozen_ppo.py:568-569 for one sample, as written there: (exp(d) - 1) - d with
// d = neglogp_new - neglogp_old (the reference's two "log_probs" are negative log-probabilities) and an exp of its own
// -- actor_loss's ratio is the exp of -d
__device__ __forceinline__ float approx_kl_term(float old_nlp, float nlp) {
  const float d = nlp - old_nlp;
  return (expf(d) - 1.0f) - d;
}

// update_mu_sigma write-back allowed?  (wave-uniform: one scalar load)
__device__ __forceinline__ bool write_back_live(const int32_t* stop) { return !(stop && stop[0] >= 0); }

// d(loss)/d(mu[q]) and d(loss)/d(sigma[q]) of one sample; g_nlp = d(loss)/d(neglogp), the coefficients already / mb
__device__ __forceinline__ float d_mu(float g_nlp, const ActionTerms& t, const ActionConsts& c, float bounds_coef_mb) {
  return g_nlp * (-(t.x / c.var)) + bounds_coef_mb * (2.0f * t.bh - 2.0f * t.blo);
}
__device__ __forceinline__ float d_sigma(float g_nlp, const ActionTerms& t, const ActionConsts& c, float entropy_coef_mb) {
  return g_nlp * (1.0f - (t.x * t.x) / c.var) - entropy_coef_mb;
}

// Shared actor-critic trunk (models_split.py:226-230: value = value(actor_mlp(x))): d(loss)/d(hidden) of one column is
// the mu heads' share CONTINUED by the value head's -- d_mu . Wmu[:, k] summed in action order, then + d_v * Wv[k] --
// times tanh' of the one hidden value both heads read.  (Two trunks: each share meets its own tanh'.)
__device__ __forceinline__ float shared_dz(float dmu_wmu, float dv, float wv, float h) {
  return fmaf(dv, wv, dmu_wmu) * (1.0f - h * h);
}

// ---------------------------------------------------------------------------------------------
// reductions of this stage only (wave_sum and dpp_mov: teacher.h)
// ---------------------------------------------------------------------------------------------
// Eight wave-wide sums at once: after the call lane l holds the sum over all 64 lanes of v[l & 7].
// Each butterfly step halves the number of live registers by keeping, per lane, only the value its low lane
// bits select (8 -> 4 -> 2 -> 1), so the whole thing is ~30 instructions instead of 8 x 11.
__device__ __forceinline__ float wave_sum8(const float (&v)[8], int lane) {
  float w[4], u[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = v[2 * j] + dpp_mov<0xB1>(v[2 * j]);          // lanes l, l^1
    const float b = v[2 * j + 1] + dpp_mov<0xB1>(v[2 * j + 1]);
    w[j] = (lane & 1) ? b : a;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float a = w[2 * i] + dpp_mov<0x4E>(w[2 * i]);          // lanes l, l^2
    const float b = w[2 * i + 1] + dpp_mov<0x4E>(w[2 * i + 1]);
    u[i] = (lane & 2) ? b : a;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {                                  // the four quads of a 16-lane row
    u[i] += dpp_mov<0x128>(u[i]);                                // row_ror:8
    u[i] += dpp_mov<0x124>(u[i]);                                // row_ror:4
  }
  float z = (lane & 4) ? u[1] : u[0];
  z += __shfl_xor(z, 16, 64);                                    // the four rows
  z += __shfl_xor(z, 32, 64);
  return z;
}
// the sum over each 16-lane row, left in all lanes of the row
__device__ __forceinline__ float rows_sum_ror(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x128>(v);   // row_ror:8 then row_ror:4: all four quads, whatever the rotate direction
  v += dpp_mov<0x124>(v);
  return v;
}
__device__ __forceinline__ float read_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// the same sum over the first 16-lane row only (k_loss: values in lanes 0..7, the rest of the row zero), returned
// wave-uniform
__device__ __forceinline__ float row0_sum(float v) { return read_lane(rows_sum_ror(v), 0); }

// ---------------------------------------------------------------------------------------------
// 2. What k_loss and k_loss_packed share.  One wave per minibatch row: lane l holds columns l, l+64, ... of the last
//    hidden layer of actor and critic, so mu/value are a wave reduction and d(hidden) leaves as one coalesced row.  Head
//    weight gradients accumulate in registers over the wave's rows and leave as one per-block partial (reduced later in
//    fixed order -> bitwise reproducible).
//    Rows are processed four at a time: lane r fetches the permutation entry of row r, then the per-sample scalars of
//    each row (actions, old mu, old sigma, advantage, return, old value, old neglogp) and the hidden rows are loaded,
//    all before any arithmetic, so a group of four rows costs two dependent memory latencies instead of eight.
// ---------------------------------------------------------------------------------------------
// rows row0 .. row0 + n - 1 of the group that starts at row `base` of a wave's share (n <= 0: nothing left; wave-uniform)
__device__ __forceinline__ int group_rows(const LossArgs& a, int row0, int base) {
  int nrows = a.rows_per_wave - base;
  if (nrows > 4) nrows = 4;
  if (nrows > a.mb - row0) nrows = a.mb - row0;
  return nrows;
}
// on lane r < nrows: the arena element of minibatch row row0 + r
__device__ __forceinline__ int group_arena_rows(const LossArgs& a, int row0, int nrows, int lane) {
  if (lane >= nrows) return 0;
  const long long b = a.perm[a.start + row0 + lane];
  const int n = (int)(b / a.T);
  return (int)(b - (long long)n * a.T) * a.N + n;  // b = n*T + t  ->  t*N + n
}

template <int MAXJ>
struct HeadTile {
  float wmu[IGI_MAX_ACT][MAXJ], wv[MAXJ];   // head weights of this lane's columns
  float gmu[IGI_MAX_ACT][MAXJ], gv[MAXJ];   // their gradients over this wave's rows

  __device__ __forceinline__ void init(const LossArgs& a, int lane) {
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int k = lane + 64 * j;
      wv[j] = (k < a.H) ? a.Wv[k] : 0.f;
      gv[j] = 0.f;
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q) {
        wmu[q][j] = (q < a.act && k < a.H) ? a.Wmu[q * a.H + k] : 0.f;
        gmu[q][j] = 0.f;
      }
    }
  }
  // this lane's columns of minibatch row `row` of both nets (zeros for a row past the end)
  static __device__ __forceinline__ void load_row(const LossArgs& a, int lane, int row, bool ok, float (&ha)[MAXJ],
                                                  float (&hc)[MAXJ]) {
    const float* ha_p = a.h + (long long)row * a.ldh;
    const float* hc_p = ha_p + a.net_stride;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int k = lane + 64 * j;
      ha[j] = (ok && k < a.H) ? ha_p[k] : 0.f;
      hc[j] = (ok && k < a.H) ? hc_p[k] : 0.f;
    }
  }
  // this lane's share of the head dot products of one row
  __device__ __forceinline__ void products(const float (&ha)[MAXJ], const float (&hc)[MAXJ], float (&pm)[IGI_MAX_ACT],
                                           float& pv) const {
    pv = 0.f;
#pragma unroll
    for (int q = 0; q < IGI_MAX_ACT; ++q) pm[q] = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      pv = fmaf(hc[j], wv[j], pv);   // explicit fma: -ffp-contract=off would issue mul + add
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q) pm[q] = fmaf(ha[j], wmu[q][j], pm[q]);
    }
  }
  // d(hidden pre-activation) of one row + its share of the head weight gradients; dmu[], dv wave-uniform
  __device__ __forceinline__ void backward_row(const LossArgs& a, int lane, int row, const float (&ha)[MAXJ],
                                               const float (&hc)[MAXJ], const float (&dmu)[IGI_MAX_ACT], float dv) {
    float* dha_p = a.dh + (long long)row * a.ld_dh;
    float* dhc_p = dha_p + a.net_stride_dh;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int k = lane + 64 * j;
      float da3 = 0.f;
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q) {
        da3 = fmaf(dmu[q], wmu[q][j], da3);
        gmu[q][j] = fmaf(dmu[q], ha[j], gmu[q][j]);
      }
      gv[j] = fmaf(dv, hc[j], gv[j]);
      if (k < a.H) {
        if (a.shared) {   // hc == ha: one row of d(pre-activation)
          dha_p[k] = shared_dz(da3, dv, wv[j], ha[j]);
        } else {
          dha_p[k] = da3 * (1.0f - ha[j] * ha[j]);
          dhc_p[k] = (dv * wv[j]) * (1.0f - hc[j] * hc[j]);
        }
      }
    }
  }
  // block partials: [muW (act*H) | muB (act) | valW (H) | valB (1) | sigma (act)] and the five loss sums
  // (actor, critic, bounds, entropy, kl) and the approx_kl sum.  Lane q < act brings d(bias_mu[q]) / d(sigma[q]), lane 0 d(bias_v) and the sums.
  __device__ __forceinline__ void store_partials(const LossArgs& a, int lane, int wave, float gbmu, float gsig, float gbv,
                                                 double s_a, double s_c, double s_b, double s_e, double s_kl, double s_ak) const {
    const int H = a.H, act = a.act;
    extern __shared__ __attribute__((aligned(16))) float red[];  // [4][head_count]
    float* mine = red + wave * a.head_count;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int k = lane + 64 * j;
      if (k < H) {
#pragma unroll
        for (int q = 0; q < IGI_MAX_ACT; ++q)
          if (q < act) mine[q * H + k] = gmu[q][j];
        mine[act * H + act + k] = gv[j];
      }
    }
    if (lane < act) {
      mine[act * H + lane] = gbmu;
      mine[act * H + act + H + 1 + lane] = gsig;
    }
    if (lane == 0) mine[act * H + act + H] = gbv;
    __shared__ double sred[LOSS_THREADS / 64][6];
    if (lane == 0) {
      sred[wave][0] = s_a; sred[wave][1] = s_c; sred[wave][2] = s_b; sred[wave][3] = s_e; sred[wave][4] = s_kl;
      sred[wave][5] = s_ak;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < a.head_count; e += blockDim.x) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < LOSS_THREADS / 64; ++w) s += red[w * a.head_count + e];
      a.head_slab[(long long)blockIdx.x * a.head_count + e] = s;
    }
    if (threadIdx.x < 6) {
      double s = 0;
      for (int w = 0; w < LOSS_THREADS / 64; ++w) s += sred[w][threadIdx.x];
      a.loss_part[blockIdx.x * 8 + threadIdx.x] = s;
    }
  }
};

// ---------------------------------------------------------------------------------------------
// 3a. act == 8 (the launcher sends every narrower action vector to k_loss_packed): lane q owns action q, the loss
//     scalars are computed redundantly on every lane and reach that (wave-uniform) arithmetic through v_readlane.
// ---------------------------------------------------------------------------------------------
template <int MAXJ>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss(const LossArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int act = a.act;
  HeadTile<MAXJ> ht;
  ht.init(a, lane);
  const bool alane = lane < act;
  const ActionConsts my = action_consts(alane ? a.logstd[lane] : 0.f);
  const float my_bmu = alane ? a.bmu[lane] : 0.f;
  float gbmu = 0.f, gsig = 0.f;         // lane q accumulates d(bias_mu[q]), d(sigma[q])
  const float bv = a.bv[0];
  float gbv = 0.f;
  double s_a = 0, s_c = 0, s_b = 0, s_e = 0, s_kl = 0, s_ak = 0;
  const bool wb = write_back_live(a.stop);
  const float inv_mb = 1.0f / (float)a.mb;
  const float lo = 1.0f - a.e_clip, hi = 1.0f + a.e_clip;

  const int gw = blockIdx.x * (LOSS_THREADS / 64) + wave;
  const int row_begin = gw * a.rows_per_wave;
  for (int base = 0; base < a.rows_per_wave; base += 4) {
    const int row0 = row_begin + base;
    const int nrows = group_rows(a, row0, base);
    if (nrows <= 0) break;  // wave-uniform
    const int my_i = group_arena_rows(a, row0, nrows, lane);
    int irow[4];
    float d[4];
    float ha[4][MAXJ], hc[4][MAXJ];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      irow[r] = __builtin_amdgcn_readlane(my_i, r);
      const long long i = irow[r];
      // lane q fetches the q-th per-sample scalar of the row.  Branch-free address select: ONE predicated load per row
      // (a chain of divergent `if (lane ...) load` arms would serialise seven dependent memory round trips)
      const float* src = a.actions + i * act + lane;
      src = (lane >= act) ? a.mus_w + i * act + (lane - act) : src;
      src = (lane >= 2 * act) ? a.sigmas_w + i * act + (lane - 2 * act) : src;
      src = (lane == 3 * act) ? a.adv + i : src;
      src = (lane == 3 * act + 1) ? a.returns_n + i : src;
      src = (lane == 3 * act + 2) ? a.values_n + i : src;
      src = (lane == 3 * act + 3) ? a.neglogpacs + i : src;
      d[r] = (r < nrows && lane < 3 * act + 4) ? *src : 0.f;
      ht.load_row(a, lane, row0 + r, r < nrows, ha[r], hc[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r >= nrows) break;  // wave-uniform
      const long long i = irow[r];
      float pm[IGI_MAX_ACT], pv;
      ht.products(ha[r], hc[r], pm, pv);
      pv = wave_sum(pv);
      float my_pm = 0.f;   // lane q ends up with its own mu[q]
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q) {
        const float t = wave_sum(pm[q]);
        my_pm = (lane == q) ? t : my_pm;
      }

      const float v = pv + bv;
      const float adv = read_lane(d[r], 3 * act), R = read_lane(d[r], 3 * act + 1), vp = read_lane(d[r], 3 * act + 2),
                  old_nlp = read_lane(d[r], 3 * act + 3);
      // per-action terms on lane q: pull the old mu / sigma of action q over from lanes act+q / 2*act+q
      const float my_mu = my_pm + my_bmu;
      ActionTerms t = action_terms(d[r], my_mu, __shfl(d[r], lane + act, 64), __shfl(d[r], lane + 2 * act, 64), my);
      t.keep_if(alane);
      const float nlp = row0_sum(t.nlp), ent = row0_sum(t.ent), bl = row0_sum(t.bl), kl = row0_sum(t.kl);
      const ActorLoss al = actor_loss(adv, old_nlp, nlp, lo, hi);
      const float g_nlp = al.dnlp * inv_mb;
      const CriticLoss cl = critic_loss(v, R, vp, a.e_clip);
      const float dv = cl.dv * (0.5f * a.critic_coef * inv_mb);

      float my_dmu = d_mu(g_nlp, t, my, a.bounds_coef * inv_mb);
      if (!alane) my_dmu = 0.f;
      if (alane) {
        gsig += d_sigma(g_nlp, t, my, a.entropy_coef * inv_mb);
        gbmu += my_dmu;
      }
      float dmu[IGI_MAX_ACT];
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q) dmu[q] = read_lane(my_dmu, q);   // back to wave-uniform for the row products
      gbv += dv;
      s_a += al.loss; s_c += cl.loss; s_b += bounds_stat(bl, a.bounds_coef); s_e += ent; s_kl += kl;
      s_ak += approx_kl_term(old_nlp, nlp);

      ht.backward_row(a, lane, row0 + r, ha[r], hc[r], dmu, dv);
      // update_mu_sigma (experience.py:228-233): scatter the new mu / sigma
      if (alane && wb) {
        a.mus_w[i * act + lane] = my_mu;
        a.sigmas_w[i * act + lane] = my.sig;
      }
    }
  }
  ht.store_partials(a, lane, wave, gbmu, gsig, gbv, s_a, s_c, s_b, s_e, s_kl, s_ak);
}

// ---------------------------------------------------------------------------------------------
// 3b. act <= 7: the per-sample scalar arithmetic done ONCE for a group of four rows.  16-lane row rr of the wave holds
//     row rr's actions / old mu / old sigma / advantage ..., its head sums land there straight out of wave_sum8, and the
//     row-local DPP sums give every row its neglogp / entropy / bounds / KL at once (the divisions, logs and exp of that
//     section were ~55 % of the per-row instruction count).
// ---------------------------------------------------------------------------------------------
template <int MAXJ>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_packed(const LossArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rr = lane >> 4, qi = lane & 15;   // scalar section: 16-lane row rr works on row rr of a group of four
  const int act = a.act;
  HeadTile<MAXJ> ht;
  ht.init(a, lane);
  // lane qi (< act) of each 16-lane row owns action dimension qi for the per-action arithmetic
  const bool alane = qi < act;
  const ActionConsts my = action_consts(alane ? a.logstd[qi] : 0.f);
  const float my_bmu = alane ? a.bmu[qi] : 0.f;
  float gbmu = 0.f, gsig = 0.f;         // lane qi accumulates d(bias_mu[qi]), d(sigma[qi])
  const float bv = a.bv[0];
  float gbv = 0.f;
  double s_a = 0, s_c = 0, s_b = 0, s_e = 0, s_kl = 0, s_ak = 0;
  const bool wb = write_back_live(a.stop);
  const float inv_mb = 1.0f / (float)a.mb;
  const float lo = 1.0f - a.e_clip, hi = 1.0f + a.e_clip;

  const int gw = blockIdx.x * (LOSS_THREADS / 64) + wave;
  const int row_begin = gw * a.rows_per_wave;
  // One group of four rows: everything it reads.  The group AFTER the one being worked on is requested first (two
  // register sets, the loop below is unrolled by two), so its two dependent round trips (permutation entry -> per-sample
  // scalars; the hidden rows do not depend on it) run under the arithmetic of the current group; only the first group
  // of a wave waits for memory.  (The mu / sigma rows written below belong to other samples than any row read later:
  // the permutation visits each sample once per pass.)
  struct LossRows {
    long long ip;
    bool okrow, aok;
    int nrows, row0;
    float ac, omu, osig, adv, R, vp, old_nlp;
    float ha[4][MAXJ], hc[4][MAXJ];
  };
  auto load_group = [&](int base, LossRows& g) {
    g.row0 = row_begin + base;
    g.nrows = group_rows(a, g.row0, base);
    if (g.nrows <= 0) return;  // wave-uniform
    const int my_i = group_arena_rows(a, g.row0, g.nrows, lane);
    // the hidden rows first: their addresses do not wait for the permutation entry
#pragma unroll
    for (int r = 0; r < 4; ++r) ht.load_row(a, lane, g.row0 + r, r < g.nrows, g.ha[r], g.hc[r]);
    // per-sample scalars in the packed layout: row rr of the group lives in 16-lane row rr
    g.okrow = rr < g.nrows;
    const long long ip = __shfl(my_i, rr, 64);
    g.ip = ip;
    g.aok = g.okrow && alane;
    g.ac = g.aok ? a.actions[ip * act + qi] : 0.f;
    g.omu = g.aok ? a.mus_w[ip * act + qi] : 0.f;
    g.osig = g.aok ? a.sigmas_w[ip * act + qi] : 0.f;
    g.adv = g.okrow ? a.adv[ip] : 0.f;
    g.R = g.okrow ? a.returns_n[ip] : 0.f;
    g.vp = g.okrow ? a.values_n[ip] : 0.f;
    g.old_nlp = g.okrow ? a.neglogpacs[ip] : 0.f;
  };
  auto compute_group = [&](const LossRows& g) {
    const bool okrow = g.okrow, aok = g.aok;
    // head dot products: after wave_sum8 EVERY lane l holds the total of value l & 7 (mu_0..mu_6, value), so row r's
    // totals are already in place for 16-lane row r -- keep them there
    float p_z = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pm[IGI_MAX_ACT], pv;
      ht.products(g.ha[r], g.hc[r], pm, pv);
      float red8[8];
#pragma unroll
      for (int q = 0; q < 7; ++q) red8[q] = pm[q];
      red8[7] = pv;
      const float z = wave_sum8(red8, lane);
      p_z = (rr == r) ? z : p_z;
    }
    // ---- scalar section, once for the four rows (lanes qi >= 8 of a row mirror lanes qi - 8: harmless)
    float my_dmu, dv;
    {
      const float pv = __shfl(p_z, (lane & 48) | 7, 64);
      const float v = pv + bv;
      const float my_mu = p_z + my_bmu;
      ActionTerms t = action_terms(g.ac, my_mu, g.omu, g.osig, my);
      t.keep_if(aok);
      const float nlp = rows_sum_ror(t.nlp), ent = rows_sum_ror(t.ent), bl = rows_sum_ror(t.bl), kl = rows_sum_ror(t.kl);
      const ActorLoss al = actor_loss(g.adv, g.old_nlp, nlp, lo, hi);
      const float g_nlp = al.dnlp * inv_mb;
      const CriticLoss cl = critic_loss(v, g.R, g.vp, a.e_clip);
      dv = okrow ? cl.dv * (0.5f * a.critic_coef * inv_mb) : 0.f;
      my_dmu = d_mu(g_nlp, t, my, a.bounds_coef * inv_mb);
      if (!aok) my_dmu = 0.f;
      if (aok) {
        gsig += d_sigma(g_nlp, t, my, a.entropy_coef * inv_mb);
        gbmu += my_dmu;
        // update_mu_sigma (experience.py:228-233): scatter the new mu / sigma
        if (wb) {
          a.mus_w[g.ip * act + qi] = my_mu;
          a.sigmas_w[g.ip * act + qi] = my.sig;
        }
      }
      if (okrow && qi == 0) {
        s_a += al.loss; s_c += cl.loss; s_b += bounds_stat(bl, a.bounds_coef); s_e += ent; s_kl += kl; gbv += dv;
        s_ak += approx_kl_term(g.old_nlp, nlp);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r >= g.nrows) break;  // wave-uniform
      float dmu[IGI_MAX_ACT];
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q) dmu[q] = read_lane(my_dmu, 16 * r + q);   // wave-uniform for the row products
      ht.backward_row(a, lane, g.row0 + r, g.ha[r], g.hc[r], dmu, read_lane(dv, 16 * r));
    }
  };
  {
    LossRows gA, gB;
    load_group(0, gA);
    for (int base = 0; base < a.rows_per_wave; base += 8) {
      if (gA.nrows <= 0) break;
      load_group(base + 4, gB);
      compute_group(gA);
      if (gB.nrows <= 0) break;
      load_group(base + 8, gA);
      compute_group(gB);
    }
  }
  // fold the four 16-lane rows' accumulators (lanes l, l ^ 16, l ^ 32, l ^ 48)
  gbmu += __shfl_xor(gbmu, 16, 64); gbmu += __shfl_xor(gbmu, 32, 64);
  gsig += __shfl_xor(gsig, 16, 64); gsig += __shfl_xor(gsig, 32, 64);
  gbv += __shfl_xor(gbv, 16, 64); gbv += __shfl_xor(gbv, 32, 64);
  s_a += __shfl_xor(s_a, 16, 64); s_a += __shfl_xor(s_a, 32, 64);
  s_c += __shfl_xor(s_c, 16, 64); s_c += __shfl_xor(s_c, 32, 64);
  s_b += __shfl_xor(s_b, 16, 64); s_b += __shfl_xor(s_b, 32, 64);
  s_e += __shfl_xor(s_e, 16, 64); s_e += __shfl_xor(s_e, 32, 64);
  s_kl += __shfl_xor(s_kl, 16, 64); s_kl += __shfl_xor(s_kl, 32, 64);
  s_ak += __shfl_xor(s_ak, 16, 64); s_ak += __shfl_xor(s_ak, 32, 64);
  ht.store_partials(a, lane, wave, gbmu, gsig, gbv, s_a, s_c, s_b, s_e, s_kl, s_ak);
}

// ---------------------------------------------------------------------------------------------
// 4.  The same loss stage fused behind the LAST trunk layer's forward (models_split.py:222-250 right behind the last
//     Linear + Tanh of :27-38; frozen_ppo.py:543-570, 618).  k_loss re-reads the 2 x mb x 128 hidden rows that layer has
//     just written (16.8 MB out, 16.8 MB in again, 16 MB of d(hidden) out) and spends one WAVE per row; here the
//     64 x 128 output tile of one net (rows m0..m0+63, actor or critic; 2 x mb / 64 workgroups, two or three per CU,
//     an actor tile paired with a critic tile) never leaves the CU:
//       A  accumulators -> LDS (the waves' 32 x 32 slices), bias + tanh in place; the head weights -> registers
//       B  head products on the matrix pipe (v_mfma_f32_16x16x4_f32): 16 rows x (<= 7 mu | value) per wave pair
//       C  the results leave the pipe as (row, action) per lane: Normal log-prob / entropy / KL / bounds with the sums over
//          the actions as 16-lane DPP sums (k_loss_packed's layout), clipped surrogate or clipped value loss with the
//          per-row scalars requested under the last k-tile, d(loss)/d(mu) | d(loss)/d(value) -> LDS, update_mu_sigma
//          write-back, bias / sigma gradient and fp64 loss sums per wave
//       D  d(pre-activation) of the layer = (d(head) . W_head) * (1 - h^2): the only large thing written to HBM (16-byte
//          row segments); head weight gradients of the tile on the matrix pipe (A = d(head)^T, B = the tanh'd tile in LDS),
//          stored straight into the tile's partial record
//       E  the waves' bias / sigma / loss partials in wave order -> the same record (mb / 64 records per minibatch)
//     The hidden layer itself is not stored (nothing reads it: the data gradient below needs tanh' of the layer BELOW).
//     The formulas are section 1's; the head sums run in the MFMA's k order.  H == 128, act <= 7;
//     other shapes (and bf16-input mode) keep the two launches.  Same box, A/B: 21.6 + 15.4 -> 30.6 us per step.
//     SHARED (cfg.shared_parameters): ONE tile per 64 rows (mb / 64 workgroups) carries both heads.  The head product has
//     act + 1 <= 8 live outputs -- mu in columns 0 .. act - 1, the value in column act -- so lane fm == act of a 16-lane row
//     runs the critic branch while lanes fm < act run the actor's; dm holds all act + 1 columns, D1 forms the one
//     d(pre-activation) row from them (shared_dz's order: the mu columns, then the value's), D2 / E fill the whole record.
// ---------------------------------------------------------------------------------------------
template <bool SHARED>
struct TrunkLossHookT {
  const LossArgs& a;
  // Per-sample scalars, requested in two steps (permutation entries up front, the rows' values under the last k-tile).  Thread (wave w, q = lane & 15, fq = lane >> 4)
  // owns action q of rows m0 + 16 (w & 3) + 4 fq + 2 (w >> 2) + r, r < 2 -- the layout in which the head products leave
  // the matrix pipe (waves w and w + 4 both compute the 16 x 16 block of rows 16 (w & 3) .. +15 and halve its rows).
  unsigned pb[2];                                   // permutation entries (step 0), then arena rows t*N + n
  float ac[2], omu[2], osig[2], s0[2], s1[2];       // (s0, s1) = (advantage, old neglogp) | (return, old value)
  float s2[2], s3[2];                               // SHARED: (s0, s1) the actor's pair, (s2, s3) = (return, old value)

  static constexpr int TILE_M = 64;                 // rows per tile: 2 x mb / 64 workgroups, two (or three) per CU
  static constexpr int EPLD = 36, SLICE = 32 * EPLD;
  static constexpr int O_DM = 8 * SLICE, O_RED = O_DM + TILE_M * 8, O_LSUM = O_RED + 8 * 16, O_LSUM5 = O_LSUM + 8 * 8,
                        O_LSUMC = O_LSUM5 + 8 * 2, LDS_FLOATS = O_LSUMC + 8 * 2;   // (O_LSUMC: SHARED's c_loss sums)

  __device__ __forceinline__ explicit TrunkLossHookT(const LossArgs& a_) : a(a_) {}

  // step 0, in front of the first tile's DMA requests: the permutation entries
  __device__ __forceinline__ void prefetch(const GemmArgs& g, int m0, int batch, int tid) {
    const int w = tid >> 6;
    const int row0 = m0 + 16 * (w & 3) + 4 * ((tid & 63) >> 4) + 2 * (w >> 2);
#pragma unroll
    for (int r = 0; r < 2; ++r) pb[r] = (unsigned)a.perm[a.start + min(row0 + r, g.M - 1)];   // < 2^31 (launcher)
  }
  // which k-tile carries step 1: the LAST one.  Requests return in order, so gathers issued in front of a tile's DMA
  // hold that tile's vmcnt wait until they have landed (issued with the first tile: +3 us per launch, with the last: +1.5;
  // measured with early exits from the kernel) -- behind the last DMA they fly under the last MFMAs and phases A / B.
  __device__ __forceinline__ int prefetch1_at(int nk) const { return nk - 1; }
  // step 1, behind the barrier of the k-tile prefetch1_at() names (the entries landed long ago)
  __device__ __forceinline__ void prefetch1(const GemmArgs& g, int batch, int tid) {
    const int q = tid & 15, act = a.act;
    // the net is wave-uniform: its two per-row arrays are picked on the scalar unit (written as an if / else over the four
    // loads the compiler built a table of the four pointers in SCRATCH and indexed it: a memory round trip in front of
    // the gathers)
    const bool actor = SHARED || batch == 0;
    const float* p0 = uniform_ptr(actor ? a.adv : a.returns_n);
    const float* p1 = uniform_ptr(actor ? a.neglogpacs : a.values_n);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const unsigned n = pb[r] / (unsigned)a.T;
      pb[r] = (pb[r] - n * (unsigned)a.T) * (unsigned)a.N + n;   // b = n*T + t  ->  t*N + n
      const long long i = pb[r];
      ac[r] = 0.f; omu[r] = 0.f; osig[r] = 1.f;
      if (actor && q < act) {
        ac[r] = a.actions[i * act + q];
        omu[r] = a.mus_w[i * act + q];
        osig[r] = a.sigmas_w[i * act + q];
      }
      s0[r] = p0[i];
      s1[r] = p1[i];
      if constexpr (SHARED) { s2[r] = a.returns_n[i]; s3[r] = a.values_n[i]; }
    }
  }

  __device__ __forceinline__ void epilogue(f32x16 (&acc)[1][1], float* smem, const GemmArgs& g, int m0, int mt, int batch,
                                           int tid, int wave, int lane, int wm, int wn) {
    typedef float f32x4r __attribute__((ext_vector_type(4)));
    const bool actor = SHARED || batch == 0;
    const int act = a.act;
    const int nq = SHARED ? act + 1 : (actor ? act : 1);   // live head outputs of this tile
    const int l31 = lane & 31, h = lane >> 5;
    const int fm = lane & 15, fq = lane >> 4;   // MFMA 16x16x4 operand / result coordinates
    const int c4 = lane & 7, rl = lane >> 3;    // row-major passes over a 64 x 32 slice: 16-byte column group, row
    float* dm = smem + O_DM;                    // [64 rows][8]: d(loss)/d(head output)
    float* red = smem + O_RED;                  // [8 waves][16]: bias / sigma gradient partials
    double* lsum = reinterpret_cast<double*>(smem + O_LSUM);   // [8 waves][4]
    double* lsum5 = reinterpret_cast<double*>(smem + O_LSUM5); // [8 waves]: the approx_kl sums
    double* lsumc = reinterpret_cast<double*>(smem + O_LSUMC); // [8 waves]: SHARED, the c_loss sums
    const float* W = actor ? a.Wmu : a.Wv;      // [nq][128] (SHARED: rows 0 .. act - 1; row act is Wv)
    // head weight row q of this tile
    auto wrow = [&](int q) { return (SHARED && q == act) ? a.Wv : W + q * 128; };
    const bool vlane = SHARED && fm == act;     // SHARED: this lane owns the value of its rows
    (void)vlane; (void)lsumc;

    // ---- A: accumulators -> this wave's slice, bias + tanh in place; meanwhile the head weights arrive in registers
    __syncthreads();   // every wave is done reading the ring
    float* ep = smem + wave * SLICE;
#pragma unroll
    for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * h) * EPLD + l31] = acc[0][0][r];
    // B operand of the head product: lane (n = fm = head output, fq) feeds W[n][16 kh + 4 fq + t] to step (kh, t)
    float4 wv[8];
#pragma unroll
    for (int kh = 0; kh < 8; ++kh)
      wv[kh] = (fm < nq) ? *reinterpret_cast<const float4*>(wrow(fm) + 16 * kh + 4 * fq) : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool alane = actor && fm < act;   // this lane owns action fm of its rows
    const float my_logstd = alane ? a.logstd[fm] : 0.f;
    const float my_bmu = alane ? a.bmu[fm] : 0.f;
    const float bvv = a.bv[0];
    const bool wb = write_back_live(a.stop);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    {
      const float4 b = *reinterpret_cast<const float4*>(g.bias + batch * g.sBias + wn * 32 + 4 * c4);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        float4* p = reinterpret_cast<float4*>(ep + (it * 8 + rl) * EPLD + 4 * c4);
        float4 v = *p;
        v.x = fast_tanh(v.x + b.x); v.y = fast_tanh(v.y + b.y); v.z = fast_tanh(v.z + b.z); v.w = fast_tanh(v.w + b.w);
        *p = v;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // ---- B: head products of rows 16 (w & 3) .. +15 on the matrix pipe (v_mfma_f32_16x16x4_f32, k = 128):
    //         A[m = fm][4 fq + t] = h[row 16 (w & 3) + fm][16 kh + 4 fq + t] (one 16-byte LDS read per four instructions)
    f32x4r hacc = f32x4r{0.f, 0.f, 0.f, 0.f};
    {
      const int row = 16 * (wave & 3) + fm;
      const float* hrow = smem + (row >> 5) * 4 * SLICE + (row & 31) * EPLD + 4 * fq;
#pragma unroll
      for (int kh = 0; kh < 8; ++kh) {
        const float4 x = *reinterpret_cast<const float4*>(hrow + (kh >> 1) * SLICE + 16 * (kh & 1));
        hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, wv[kh].x, hacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, wv[kh].y, hacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, wv[kh].z, hacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, wv[kh].w, hacc, 0, 0, 0);
      }
    }
    // ---- C: hacc[2 (w >> 2) + r] = head output fm of row 16 (w & 3) + 4 fq + 2 (w >> 2) + r: this lane's action of its
    //         two rows.  The sums over the actions of a row are sums over the 16-lane row (DPP), as in k_loss_packed.
    float gb = 0.f, gs = 0.f;            // d(bias_mu[fm]) | d(bias_v), d(sigma[fm]) over this lane's rows
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, tc = 0;
    {
      const float inv_mb = 1.0f / (float)a.mb;
      const ActionConsts my = action_consts(my_logstd);
      const float lo = 1.0f - a.e_clip, hi = 1.0f + a.e_clip;
      const int hi2 = wave >> 2;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int rowt = 16 * (wave & 3) + 4 * fq + 2 * hi2 + r;           // row of the tile
        const bool okrow = m0 + rowt < g.M;
        const float hout = hi2 ? hacc[2 + r] : hacc[r];
        float my_d = 0.f;
        if (actor) {
          const bool aok = okrow && alane;
          const float my_mu = hout + my_bmu;
          ActionTerms t = action_terms(ac[r], my_mu, omu[r], osig[r], my);
          t.keep_if(aok);
          const float nlp = rows_sum_ror(t.nlp), ent = rows_sum_ror(t.ent), bl = rows_sum_ror(t.bl), kl = rows_sum_ror(t.kl);
          const ActorLoss al = actor_loss(s0[r], s1[r], nlp, lo, hi);
          const float g_nlp = al.dnlp * inv_mb;
          if (aok) {
            my_d = d_mu(g_nlp, t, my, a.bounds_coef * inv_mb);
            gs += d_sigma(g_nlp, t, my, a.entropy_coef * inv_mb);
            gb += my_d;
            // update_mu_sigma (experience.py:228-233): scatter the new mu / sigma
            if (wb) {
              a.mus_w[(long long)pb[r] * act + fm] = my_mu;
              a.sigmas_w[(long long)pb[r] * act + fm] = my.sig;
            }
          }
          if (okrow && fm == 0) {
            t0 += al.loss; t1 += bounds_stat(bl, a.bounds_coef); t2 += ent; t3 += kl;
            t4 += approx_kl_term(s1[r], nlp);
          }
          if constexpr (SHARED) {   // the critic branch on the lane that holds the value (no action of its own: my_d == 0 so far)
            const CriticLoss cl = critic_loss(hout + bvv, s2[r], s3[r], a.e_clip);
            if (okrow && vlane) {
              my_d = cl.dv * (0.5f * a.critic_coef * inv_mb);
              gb += my_d;
              tc += cl.loss;
            }
          }
        } else {
          const CriticLoss cl = critic_loss(hout + bvv, s0[r], s1[r], a.e_clip);
          if (okrow && fm == 0) {
            my_d = cl.dv * (0.5f * a.critic_coef * inv_mb);
            gb += my_d;
            t0 += cl.loss;
          }
        }
        if (fm < 8) dm[rowt * 8 + fm] = my_d;
      }
      // this wave's 8 rows: lanes fm, fm + 16, fm + 32, fm + 48
      gb += __shfl_xor(gb, 16, 64); gb += __shfl_xor(gb, 32, 64);
      gs += __shfl_xor(gs, 16, 64); gs += __shfl_xor(gs, 32, 64);
      t0 += __shfl_xor(t0, 16, 64); t0 += __shfl_xor(t0, 32, 64);
      if (actor) {
        t1 += __shfl_xor(t1, 16, 64); t1 += __shfl_xor(t1, 32, 64);
        t2 += __shfl_xor(t2, 16, 64); t2 += __shfl_xor(t2, 32, 64);
        t3 += __shfl_xor(t3, 16, 64); t3 += __shfl_xor(t3, 32, 64);
        t4 += __shfl_xor(t4, 16, 64); t4 += __shfl_xor(t4, 32, 64);
      }
      if constexpr (SHARED) { tc += __shfl_xor(tc, 16, 64); tc += __shfl_xor(tc, 32, 64); }
      if (lane < 8) { red[wave * 16 + lane] = gb; red[wave * 16 + 8 + lane] = gs; }
      if (lane == 0) {
        lsum[wave * 4 + 0] = t0; lsum[wave * 4 + 1] = t1; lsum[wave * 4 + 2] = t2; lsum[wave * 4 + 3] = t3;
        lsum5[wave] = t4;
      }
      if (SHARED && lane == act) lsumc[wave] = tc;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // LDS-only rendezvous: the mu / sigma stores stay in flight
    asm volatile("" ::: "memory");

    // ---- D1: d(pre-activation) of this wave's 32 x 32 slice = (d(head) . W_head) * (1 - h^2), 16-byte row segments
    {
      constexpr int NQ = SHARED ? 8 : 7;
      float4 w[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        w[q] = (q < nq) ? *reinterpret_cast<const float4*>(wrow(q) + wn * 32 + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      float* dst = a.dh + batch * a.net_stride_dh + (long long)(m0 + wm * 32) * a.ld_dh + wn * 32 + 4 * c4;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int r = it * 8 + rl;
        const float4 hv = *reinterpret_cast<const float4*>(ep + r * EPLD + 4 * c4);
        const float4 d0 = *reinterpret_cast<const float4*>(dm + (wm * 32 + r) * 8);
        const float4 d1 = *reinterpret_cast<const float4*>(dm + (wm * 32 + r) * 8 + 4);
        const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          if (q < nq) {
            z.x = fmaf(d[q], w[q].x, z.x); z.y = fmaf(d[q], w[q].y, z.y);
            z.z = fmaf(d[q], w[q].z, z.z); z.w = fmaf(d[q], w[q].w, z.w);
          }
        z.x = z.x * (1.0f - hv.x * hv.x); z.y = z.y * (1.0f - hv.y * hv.y);
        z.z = z.z * (1.0f - hv.z * hv.z); z.w = z.w * (1.0f - hv.w * hv.w);
        if (m0 + wm * 32 + r < g.M) *reinterpret_cast<float4*>(dst + (long long)r * a.ld_dh) = z;
      }
    }
    // ---- D2: head weight gradients of columns 16 w .. 16 w + 15 over the tile's 64 rows, on the matrix pipe:
    //          out[q][col] = sum_row dm[row][q] * h[row][col];  A[m = q][4 fq + t] = dm[16 st + 4 fq + t][q],
    //          B[4 fq + t][n = col] = h[16 st + 4 fq + t][16 w + n]
    {
      f32x4r gacc = f32x4r{0.f, 0.f, 0.f, 0.f};
      const int col = 16 * wave + fm;
      const float* hcol = smem + (col >> 5) * SLICE + (col & 31);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        float av[4], bvv4[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int row = 16 * st + 4 * fq + t;
          av[t] = (fm < 8) ? dm[row * 8 + fm] : 0.f;
          bvv4[t] = hcol[(row >> 5) * 4 * SLICE + (row & 31) * EPLD];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bvv4[t], gacc, 0, 0, 0);
      }
      // gacc[r] = out[q = 4 fq + r][col]; record mt: [muW (act*H) | muB (act) | valW (H) | valB (1) | sigma (act)]
      float* rec = a.head_slab + (long long)mt * a.head_count;
      if (actor) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (4 * fq + r < act) rec[(4 * fq + r) * 128 + col] = gacc[r];
          else if (SHARED && 4 * fq + r == act) rec[act * 128 + act + col] = gacc[r];   // valW
        }
      } else if (fq == 0) {
        rec[act * 128 + act + col] = gacc[0];
      }
    }
    // ---- E: the waves' bias / sigma / loss partials in wave order
    if (tid < 16) {
      float sb = 0.f;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) sb += red[w8 * 16 + tid];
      float* rec = a.head_slab + (long long)mt * a.head_count;
      if (actor) {
        if (tid < act) rec[act * 128 + tid] = sb;                                          // muB
        else if (SHARED && tid == act) rec[act * 128 + act + 128] = sb;                    // valB (act <= 7: a lane below 8)
        else if (tid >= 8 && tid - 8 < act) rec[act * 128 + act + 128 + 1 + (tid - 8)] = sb;   // sigma
      } else if (tid == 0) {
        rec[act * 128 + act + 128] = sb;                                                    // valB
      }
    } else if (tid >= 64 && tid < 68) {
      const int j = tid - 64;
      double sl = 0;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) sl += lsum[w8 * 4 + j];
      double* lp = a.loss_part + (long long)mt * 8;
      if (actor) lp[j == 0 ? 0 : j + 1] = sl;     // a_loss, bounds, entropy, kl -> slots 0, 2, 3, 4
      else if (j == 0) lp[1] = sl;                // c_loss -> slot 1
    } else if (tid == 68 && actor) {
      double sl = 0;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) sl += lsum5[w8];
      a.loss_part[(long long)mt * 8 + 5] = sl;    // approx_kl -> slot 5
    } else if (SHARED && tid == 69) {
      double sl = 0;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) sl += lsumc[w8];
      a.loss_part[(long long)mt * 8 + 1] = sl;    // c_loss -> slot 1
    }
  }
};
typedef TrunkLossHookT<false> TrunkLossHook;

template <bool SHARED>
__global__ __launch_bounds__(DMA_THREADS, 4) void k_trunk_loss(const GemmArgs g, const LossArgs a, int m_tiles) {
  TrunkLossHookT<SHARED> hook(a);
  // no XCD remap: workgroup b and b + m_tiles (the same rows of the other net) land on the same XCD, and the round-robin
  // placement pairs an actor tile with a critic tile on a CU (the actor's scalar section is the longer one)
  gemm_dma_body<128, true, true, 0, 2, TrunkLossHook::TILE_M, false, false, false, false, TrunkLossHookT<SHARED>>(
      g, 1, m_tiles, (int)blockIdx.x, &hook);
}

// ---------------------------------------------------------------------------------------------
// 5. The stage of one minibatch.  d(pre-activation) of the last trunk layer leaves in the layout (ld_dh, net_stride_dh)
//    the trunk backward reads it in.
// ---------------------------------------------------------------------------------------------
static int loss_stage(const TeacherPlan& p, const igi_teacher_cfg* c, const igi_rollout* ro, const igi_teacher_state* st,
                      int mb_index, int ld_dh, long long net_stride_dh, hipStream_t s, const int32_t* stop = nullptr) {
  const float* P = st->params;
  const int mb = p.mb;
  const long long mbs = mb;
  const int H = p.u[p.nl - 1];
  const int ldh = ru4(H);
  LossArgs a;
  a.h = wsp<float>(st, p.w_h[p.nl - 1]);
  a.dh = wsp<float>(st, p.w_dh[p.nl - 1]);
  a.shared = p.nets == 1;
  a.net_stride = a.shared ? 0 : mbs * ldh; a.ldh = ldh; a.H = H;
  a.ld_dh = ld_dh; a.net_stride_dh = net_stride_dh;
  a.Wmu = P + p.o_muW; a.bmu = P + p.o_muB; a.Wv = P + p.o_valW; a.bv = P + p.o_valB;
  a.logstd = P + p.o_sigma;
  a.actions = ro->actions; a.neglogpacs = ro->neglogpacs;
  a.adv = st->advantages; a.values_n = st->values_n; a.returns_n = st->returns_n;
  a.mus_w = st->mus_w; a.sigmas_w = st->sigmas_w;
  a.perm = st->perm; a.start = (long long)mb_index * mb;
  a.mb = mb; a.N = p.N; a.T = p.T; a.act = p.act; a.rows_per_wave = p.loss_rpw;
  a.e_clip = c->e_clip; a.critic_coef = c->critic_coef; a.entropy_coef = c->entropy_coef;
  a.bounds_coef = c->bounds_loss_coef;
  a.loss_part = wsp<double>(st, p.w_loss_part);
  a.stop = stop;
  a.head_slab = wsp<float>(st, p.w_head_slab);
  a.head_count = p.head_count;
  if (p.loss_fused) {
    // last trunk layer (both nets) with the heads, the loss and the head backward in its tiles' epilogue
    const int l = p.nl - 1, in = ac_in(p, l);
    GemmArgs g;
    g.A = wsp<float>(st, p.w_h[l - 1]); g.lda = ru4(in); g.sA = mbs * ru4(in);
    g.B = P + p.o_acW[l]; g.ldb = in; g.sB = p.ac_block; g.K = in;
    g.bias = P + p.o_acB[l]; g.sBias = p.ac_block;
    g.M = mb; g.N = H; g.nbatch = p.nets;
    g.epilogue = EPI_BIAS_TANH;
    if (!dma_eligible(g, true, true) || !aligned16(g.bias) || (g.sBias & 3) || !aligned16(a.dh) || (a.ld_dh & 3) ||
        (a.net_stride_dh & 3))
      return IGI_E_UNSUPPORTED;
    const int m_tiles = (mb + TrunkLossHook::TILE_M - 1) / TrunkLossHook::TILE_M;
    dma_set_divs(g, 1, m_tiles);
    constexpr size_t ring = sizeof(float) * 2 * (TrunkLossHook::TILE_M + 128) * DMA_BK;
    constexpr size_t shm = sizeof(float) * TrunkLossHook::LDS_FLOATS > ring ? sizeof(float) * TrunkLossHook::LDS_FLOATS : ring;
    static bool attr[2] = {false, false};
    if (!attr[a.shared]) {
      const void* fn = a.shared ? (const void*)k_trunk_loss<true> : (const void*)k_trunk_loss<false>;
      IGI_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
      attr[a.shared] = true;
    }
    const double nn = p.nets;
    ProfScope ps(PC_TRUNK_LOSS, s, 2.0 * nn * (double)mbs * H * in + 2.0 * 3 * (double)mbs * H * (p.act + 1),
                 4.0 * (nn * mbs * in + nn * H * in + nn * mbs * H + (double)mbs * (4 * p.act + 6)));
    // shared trunk: ONE tile per 64 rows carries both heads
    if (a.shared) IGI_LAUNCH(k_trunk_loss<true>, dim3(m_tiles), dim3(DMA_THREADS), shm, s, g, a, m_tiles);
    else IGI_LAUNCH(k_trunk_loss<false>, dim3(2 * m_tiles), dim3(DMA_THREADS), shm, s, g, a, m_tiles);
    return 0;
  }
  ProfScope ps(PC_LOSS, s, 2.0 * 3 * (double)mbs * H * (p.act + 1), 4.0 * (double)mbs * (4.0 * ldh + 4 * p.act + 6));
  const size_t shm = sizeof(float) * 4 * p.head_count;
  if (p.act <= 7) IGI_LAUNCH_MAXJ(k_loss_packed, H, dim3(p.loss_blocks), dim3(LOSS_THREADS), shm, s, a);
  else IGI_LAUNCH_MAXJ(k_loss, H, dim3(p.loss_blocks), dim3(LOSS_THREADS), shm, s, a);
  return 0;
}

}  // namespace igi
