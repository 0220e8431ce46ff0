// Teacher PPO update on gfx950: rollout post-processing (GAE, advantage / value normalisation),
// minibatch gather + running-stat update, fused policy/value heads + PPO loss + head backward,
// deterministic split-K gradient reduction, global-norm clip + Adam.
//
// Data layout in HBM
//   * rollout arena stays time-major [t][n][.] exactly as play_steps wrote it; the reference's
//     env-major sample id b = n*T + t (experience.py:39-46) is mapped to element t*N + n on the fly,
//     so the 11 transpose-copies of prepare_training never happen;
//   * parameters / gradients / Adam moments are single flat fp32 vectors in state_dict order;
//   * per-minibatch activations are row-major [mb][width4] (width rounded up to 4 floats so rows
//     are 16-byte aligned), actor and critic stacked [nets][mb][width4] so one batched launch serves both
//     (nets = 1 with a shared actor-critic trunk: cfg.shared_parameters).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "../../include/igi_ppo.h"
#include "gemm_dma.h"
#include "rowblock.h"
#include "env_mlp.h"
#include "policy_fwd.h"
#include "fwd12.h"
#include "gemm_f32.h"
#include "rollout.h"
#include "contact.h"

namespace igi {

#define IGI_HIP_TRY(expr)                      \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return (int)_e;      \
  } while (0)

static inline int ru4(int x) { return (x + 3) & ~3; }
static inline long long ru64(long long x) { return (x + 63) & ~63LL; }  // 256-byte granules

constexpr int PREP_THREADS = 256;
constexpr int GS_THREADS = 256;
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_BLOCKS_DEFAULT = 512;  // measured: 256 -> 55 us, 512 -> 35 us, 1024 -> 37 us per launch
constexpr int RED_THREADS = 256;
constexpr int SUMSQ_BLOCKS = 512;
// Segments of the flat-gradient assembly (assemble_gradient), worst case of what make_plan accepts, for L layers per MLP:
// 4 heads (mu W, b; value W, b) + 1 sigma + 2 per env_mlp layer (W, b; the fused latent level's two records stand in for the
// last layer's) + 4 contact encoder (W1, b1, W2, b2) + 4 per trunk layer (W, b of actor and critic) = 9 + 6 L; L = 4: 33.
constexpr int teacher_max_segments(int max_layers) { return 4 + 1 + 2 * max_layers + 4 + 4 * max_layers; }
constexpr int MAX_SEG = 33;
static_assert(MAX_SEG >= teacher_max_segments(IGI_MAX_LAYERS),
              "SegTable cannot hold the gradient segments of the largest network make_plan accepts: raise MAX_SEG");
constexpr int ADAM_BLOCKS_MAX = 1024;

// ---------------------------------------------------------------------------------------------
// plan: parameter offsets + workspace carve-up, recomputed from the cfg on every call (pure
// integer arithmetic on the host).
// ---------------------------------------------------------------------------------------------
struct TeacherPlan {
  int obs, priv, act, npl, nl;
  int nets;             // trunks: 2 = actor_mlp + critic_mlp, 1 = shared_parameters (value reads the actor trunk's output)
  int pu[IGI_MAX_LAYERS], u[IGI_MAX_LAYERS];
  int N, T, E, mb, nmb;
  long long Bsz;
  int latent, xw, xld;  // xcat = [obs_n | latent | 0...], width xw, leading dim xld (multiple of 32)
  // ground-truth contacts (cfg contact_points > 0): xcat = [obs_n | latent | contact embedding | 0...], or
  // [obs_n | contact embedding | 0...] with only_contact (env_mlp is then neither run nor trained)
  int ct_P, ct_E, ct_only, ct_col, ct_blocks;
  long long o_ctW1, o_ctB1, o_ctW2, o_ctB2, o_cdW1, o_cdB1, o_cdW2, o_cdB2, ct_rec;
  size_t w_ct_h, w_ct_part;
  int u0p;              // first trunk width rounded up to 4
  // parameter offsets (floats) in the flat vector
  long long o_sigma, o_envW[IGI_MAX_LAYERS], o_envB[IGI_MAX_LAYERS];
  long long o_acW[IGI_MAX_LAYERS], o_acB[IGI_MAX_LAYERS];  // actor; critic = + ac_block (nets == 2)
  long long ac_block, o_valW, o_valB, o_muW, o_muB, P;
  // workspace offsets (bytes)
  size_t w_prep_part, w_prep_coef, w_rms_part, w_norm_coef, w_priv, w_xcat, w_dxcat, w_w1p;
  size_t w_moments, w_traj_coef, w_traj_state, w_lat_part, w_wlat, w_lat_rowdot;
  int lat_tiles;
  int lat_fused, lat_blocks, lat_rpw;  // fused latent / last-env-layer backward (k_latent_bwd)  // per-minibatch batch moments; per-step normaliser trajectory
  size_t w_e[IGI_MAX_LAYERS], w_de[IGI_MAX_LAYERS], w_h[IGI_MAX_LAYERS], w_dh[IGI_MAX_LAYERS];
  size_t w_loss_part, w_head_slab, w_slab, w_sumsq, w_scal, w_total;
  int gae_blocks, gs_rows, gs_blocks, loss_blocks, loss_rpw;
  int loss_fused;  // heads + loss + head backward ride in the last trunk layer's forward (k_trunk_loss); loss_blocks = its m-tiles
  // backward levels that run as ONE persistent row-block kernel (rowblock.h) instead of data-gradient + weight-gradient
  // tiles: rb_ac[l] / rb_env[l] = row ranges (= weight-gradient partials) of trunk / env_mlp layer l, 0 = tile kernels
  int rb_ac[IGI_MAX_LAYERS], rb_env[IGI_MAX_LAYERS];
  // the FIRST trunk layer's weight gradient comes from the data-gradient tiles that produce its dZ (GemmArgs::lw_*):
  // lw_chain consecutive row tiles per workgroup, lw_parts partial records per net; dZ of that layer is never written
  int lw_chain, lw_parts;
  int lx_env;   // the FIRST env layer's weight gradient rides in the env level's row-block kernel (rowblock.h, LOWX); its dZ is never written
  int latz;     // round 6 (IGI_LATZ_FUSE=0 turns it off): k_latent_bwd's work at the head of the env level's blocks (rowblock.h, LATZ); de2 is never written
  int head_count;  // muW, muB, valW, valB, sigma partial vector length
  // wgrad split factors and slab offsets (floats, relative to w_slab)
  int sk_env[IGI_MAX_LAYERS], sk_ac[IGI_MAX_LAYERS];
  long long s_envW[IGI_MAX_LAYERS], s_envB[IGI_MAX_LAYERS], s_acW[IGI_MAX_LAYERS], s_acB[IGI_MAX_LAYERS];
  long long slab_floats;
};

static inline int env_in(const TeacherPlan& p, int l) { return l == 0 ? p.priv : p.pu[l - 1]; }
static inline int ac_in(const TeacherPlan& p, int l) { return l == 0 ? p.xw : p.u[l - 1]; }
// d(pre-activation) of trunk layer l: stacked [net][mb][width4] like the activations, except the FIRST layer's, which is
// kept interleaved [row][net][u0p] so that the data gradient into xcat is one contraction over both nets
static inline int dz_ld(const TeacherPlan& p, int l) { return l == 0 ? p.nets * p.u0p : ru4(p.u[l]); }
static inline long long dz_stride(const TeacherPlan& p, int l) { return l == 0 ? (long long)p.u0p : (long long)p.mb * ru4(p.u[l]); }
static inline bool H_last_is_128(const TeacherPlan* p) { return p->u[p->nl - 1] == 128; }

static int choose_splitk(int M, int N, int K, int nbatch) {
  if (M >= 4 && N >= 4 && (M & 3) == 0 && (N & 3) == 0) {
    // the weight gradients run in gemm_dma_wgrad_multi_kernel: 128 x 128 tiles (128 x 64 up to 64 input columns).  One
    // workgroup per CU and product: with the tile width that kernel really uses (the generic planner assumes 256-wide
    // tiles for wide layers and gave the 512 -> 256 layer 32 splits = 512 workgroups of 16 k-tiles; 16 splits = 256
    // workgroups of 32 k-tiles, first in the grid, halve its slab and run 7 us shorter)
    const int bn = N <= 64 ? 64 : 128;
    // (<= 32 input columns and whole 256-row tiles: gemm_wgrad_multi runs 256 x 32 tiles, kind 3)
    const int bm = (N <= 32 && M % 256 == 0) ? 256 : DMA_BM;
    const long long tiles = (long long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * nbatch;
    int sk = (int)(256 / tiles > 1 ? 256 / tiles : 1);
    const int maxsk = K / 128 > 1 ? K / 128 : 1;
    return sk > maxsk ? maxsk : sk;
  }
  int bm, bn;
  gemm_tile_for(M, N, &bm, &bn);
  long long tiles = (long long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * nbatch;
  int sk = (int)((256 + tiles - 1) / tiles);
  int maxsk = K / 128;
  if (sk > maxsk) sk = maxsk;
  if (sk < 1) sk = 1;
  return sk;
}

// igi_teacher_set_latz_fuse / IGI_LATZ_FUSE (initial value).  Default ON since the rank-8 weight gradient of the block runs
// on the matrix pipe (rowblock.h, latz_head): alternating A/B on one box (profiles/r06_latz_ab.log) 38.71 / 39.40 / 39.87
// updates/s on against 38.60 / 38.52 / 38.92 off -- the 9.0 us launch it removes (k_latent_bwd) and ~1.3 us of the slab sum /
// Adam pass against +4.5 us in the env level (36.1 - 39.3 -> 39.5 - 44.9 us; the transform of the staged image is vector work
// that the four column slices of a row range repeat, behind two more barriers per block).  With that phase as vector code
// (64 LDS reads and ~45 address instructions per 8 rows and thread) the two were even: 39.16 / 39.25 on, 39.16 / 39.23 off.
// The workspace carve-up does not depend on the switch.
static inline int& latz_fuse_ref() {
  static int on = -1;
  if (on < 0) { const char* e = getenv("IGI_LATZ_FUSE"); on = e ? (atoi(e) != 0) : 1; }
  return on;
}
// IGI_ENV_FUSED=0, a test seam (the bit-equality tests run both settings in child processes): the env_mlp forward layer by
// layer instead of k_env_fwd / k_fwd12
static inline int env_fused() {
  static int on = -1;
  if (on < 0) { const char* e = getenv("IGI_ENV_FUSED"); on = e ? atoi(e) : 1; }
  return on;
}

static int make_plan(const igi_teacher_cfg* c, TeacherPlan* p) {
  memset(p, 0, sizeof(*p));
  if (!c) return IGI_E_BADARG;
  if (c->n_priv_layers < 1 || c->n_priv_layers > IGI_MAX_LAYERS || c->n_layers < 1 ||
      c->n_layers > IGI_MAX_LAYERS || c->act_dim < 1 || c->act_dim > IGI_MAX_ACT ||
      c->obs_dim < 1 || c->priv_dim < 1 || c->num_envs < 1 || c->horizon < 1 || c->mini_epochs < 1)
    return IGI_E_BADARG;
  p->obs = c->obs_dim; p->priv = c->priv_dim; p->act = c->act_dim;
  p->npl = c->n_priv_layers; p->nl = c->n_layers;
  for (int i = 0; i < p->npl; ++i) { p->pu[i] = c->priv_units[i]; if (p->pu[i] < 1) return IGI_E_BADARG; }
  for (int i = 0; i < p->nl; ++i) { p->u[i] = c->units[i]; if (p->u[i] < 1) return IGI_E_BADARG; }
  if (p->u[p->nl - 1] > 256) return IGI_E_UNSUPPORTED;  // head kernel keeps <=4 columns per lane
  p->N = c->num_envs; p->T = c->horizon; p->E = c->mini_epochs;
  p->Bsz = (long long)p->N * p->T;
  p->mb = (int)(p->Bsz / p->E);
  if (p->mb < 2) return IGI_E_BADARG;
  p->nmb = (int)(p->Bsz / p->mb);
  p->latent = p->pu[p->npl - 1];
  if (c->shared_parameters != 0 && c->shared_parameters != 1) return IGI_E_BADARG;
  p->nets = c->shared_parameters ? 1 : 2;
  p->ct_P = c->contact_points; p->ct_E = c->contact_emb; p->ct_only = c->only_contact;
  if (p->ct_P < 0 || p->ct_E < 0 || p->ct_only < 0 || p->ct_only > 1) return IGI_E_BADARG;
  if (p->ct_P == 0 && (p->ct_E != 0 || p->ct_only)) return IGI_E_BADARG;
  if (p->ct_P > 0 && (p->ct_E < 1 || p->ct_E > CT_MAX_EMB)) return IGI_E_BADARG;
  if (p->ct_only && p->ct_E != p->latent) return IGI_E_UNSUPPORTED;   // the reference's trunk width is obs + latent
  if (p->nets == 1 && p->ct_P > 0) return IGI_E_UNSUPPORTED;          // shared_parameters with compute_contact_gt
  p->ct_col = p->obs + (p->ct_only ? 0 : p->latent);
  p->xw = p->ct_col + p->ct_E;
  p->xld = (p->xw + 31) & ~31;  // zero-padded to the LDS-DMA kernel's k-tile
  p->u0p = ru4(p->u[0]);

  // every tensor starts on a 16-byte boundary (gaps stay zero) so weight tiles load as float4
  long long o = 0;
  auto put = [&](long long n) { long long at = o; o = (o + n + 3) & ~3LL; return at; };
  p->o_sigma = put(p->act);
  for (int l = 0; l < p->npl; ++l) {
    p->o_envW[l] = put((long long)p->pu[l] * env_in(*p, l));
    p->o_envB[l] = put(p->pu[l]);
  }
  if (p->ct_P > 0) {   // contact_ae: encoder then decoder, state_dict order (models_split.py:45-47)
    p->o_ctW1 = put((long long)CT_HID * p->ct_P); p->o_ctB1 = put(CT_HID);
    p->o_ctW2 = put((long long)p->ct_E * CT_HID); p->o_ctB2 = put(p->ct_E);
    p->o_cdW1 = put((long long)CT_HID * p->ct_E); p->o_cdB1 = put(CT_HID);
    p->o_cdW2 = put((long long)p->ct_P * CT_HID); p->o_cdB2 = put(p->ct_P);
  }
  long long ac0 = o;
  for (int l = 0; l < p->nl; ++l) {
    p->o_acW[l] = put((long long)p->u[l] * ac_in(*p, l));
    p->o_acB[l] = put(p->u[l]);
  }
  p->ac_block = o - ac0;
  o += (p->nets - 1) * p->ac_block;  // critic: same shapes, same internal offsets
  const int H = p->u[p->nl - 1];
  p->o_valW = put(H);
  p->o_valB = put(1);
  p->o_muW = put((long long)p->act * H);
  p->o_muB = put(p->act);
  p->P = o;

  // ---- workspace
  const long long mb = p->mb;
  size_t w = 0;
  auto take = [&](size_t bytes) { size_t at = w; w += (size_t)ru64((long long)bytes); return at; };
  p->gae_blocks = (p->N + PREP_THREADS - 1) / PREP_THREADS;
  p->w_prep_part = take(sizeof(double) * 6 * p->gae_blocks);
  p->w_prep_coef = take(sizeof(float) * 8);
  const int D = p->obs + p->priv;
  p->gs_rows = 32;
  while (p->gs_rows > 8 && (size_t)p->gs_rows * (D + 2) * sizeof(float) > 48 * 1024) p->gs_rows /= 2;
  p->gs_blocks = (int)((mb + p->gs_rows - 1) / p->gs_rows);
  p->w_rms_part = take(sizeof(double) * 2 * D * p->gs_blocks * p->nmb);
  p->w_norm_coef = take(sizeof(float) * 2 * D);
  p->w_moments = take(sizeof(float) * 2 * D * p->nmb);
  p->w_traj_coef = take(sizeof(float) * 2 * D * p->E * p->nmb);
  p->w_traj_state = take(sizeof(double) * (2 * D + 2) * p->E * p->nmb);
  {
    const int K2 = p->nets * ru4(p->u[0]);
    // LDS: transposed weight slice 8 x (K2p+4) + 32 x 260 staging tile (also hosts the 4 x (8*H2+8) final reduction)
    p->lat_fused = (p->latent == 8 && p->ct_P == 0 && p->npl >= 2 && p->pu[p->npl - 2] <= 256 && K2 <= 2048) ? 1 : 0;
    p->lat_rpw = 0;
    p->lat_blocks = (int)((mb + 31) / 32);
    p->w_lat_part = p->lat_fused ? take(sizeof(float) * (size_t)p->lat_blocks * (8 * p->pu[p->npl - 2] + 8)) : 0;
    // row dots of dZ1 with the eight latent columns, one partial per 128-column tile and net (see k_latent_bwd<., true>)
    p->lat_tiles = p->nets * ((p->u[0] + 127) / 128);
    p->w_lat_rowdot = p->lat_fused ? take(sizeof(float) * (size_t)p->lat_tiles * mb * 8) : 0;
    p->w_wlat = p->lat_fused ? take(sizeof(float) * 8 * (size_t)((K2 + 255) / 256 * 256)) : 0;  // [8][K2p], see k_latent_bwd
  }
  p->w_priv = take(sizeof(float) * mb * ru4(p->priv));
  p->w_xcat = take(sizeof(float) * mb * p->xld);
  p->w_dxcat = take(sizeof(float) * mb * p->xld);
  p->w_w1p = take(sizeof(float) * p->nets * p->u0p * p->xld);
  if (p->ct_P > 0) {
    p->ct_blocks = ct_bwd_blocks(p->mb);
    p->ct_rec = ct_rec_floats(p->ct_P, p->ct_E);
    p->w_ct_h = take(sizeof(float) * mb * CT_HID);
    p->w_ct_part = take(sizeof(float) * (size_t)p->ct_blocks * p->ct_rec);
  }
  for (int l = 0; l < p->npl; ++l) {
    // rows rounded up to the fused env_mlp kernel's 64-row blocks: it stores whole blocks (env_mlp.h)
    p->w_e[l] = (l < p->npl - 1) ? take(sizeof(float) * ((mb + 63) / 64 * 64) * ru4(p->pu[l])) : 0;
    p->w_de[l] = (l < p->npl - 1) ? take(sizeof(float) * mb * ru4(p->pu[l])) : 0;  // last: dxcat[:, obs:]
  }
  for (int l = 0; l < p->nl; ++l) {
    p->w_h[l] = take(sizeof(float) * p->nets * mb * ru4(p->u[l]));
    p->w_dh[l] = take(sizeof(float) * p->nets * mb * ru4(p->u[l]));
  }
  // loss kernel: one wave per row, loss_rpw rows per wave
  long long waves_needed = mb;
  int blocks = (int)((waves_needed + 4 * 4 - 1) / (4 * 4));
  if (blocks > LOSS_BLOCKS_DEFAULT) blocks = LOSS_BLOCKS_DEFAULT;
  if (blocks < 1) blocks = 1;
  p->loss_blocks = blocks;
  p->loss_rpw = (int)((mb + (long long)blocks * 4 - 1) / ((long long)blocks * 4));
  {
    // the fused last-layer forward + loss (k_trunk_loss): decided from the shapes alone, so that the workspace carve-up,
    // the slab sums and the statistics kernel agree on the number of partial records (one per 64-row m-tile)
    // (the launch site re-checks dma_eligible and the 16-byte alignment of bias / dh: every offset and stride that enters
    // those checks is tested HERE, so that a shape which passes keeps passing at the launch and one which does not keeps
    // the two-launch path -- only a misaligned base pointer of the caller remains an error there)
    const int ll = p->nl - 1;
    const bool aligned = (p->o_acW[ll] & 3) == 0 && (p->o_acB[ll] & 3) == 0 && (p->ac_block & 3) == 0 &&
                         (ru4(p->u[ll]) & 3) == 0 && (ru4(p->u[ll - (ll > 0)]) & 3) == 0 && ((long long)p->mb * ru4(p->u[ll]) & 3) == 0;
    p->loss_fused = (p->nl >= 2 && H_last_is_128(p) && p->act <= 7 && (p->u[p->nl - 2] % DMA_BK) == 0 &&
                     p->Bsz < (1LL << 31) && !bf16_mode() && aligned) ? 1 : 0;
    if (p->loss_fused) p->loss_blocks = (int)((mb + 63) / 64);   // TrunkLossHook::TILE_M
  }
  p->w_loss_part = take(sizeof(double) * 8 * p->loss_blocks);
  p->head_count = p->act * H + p->act + H + 1 + p->act;
  p->w_head_slab = take(sizeof(float) * (size_t)p->head_count * p->loss_blocks);
  // wgrad slabs.  Every product picks its split factor as if it had the chip to itself (power-of-two k-chunks).
  // Planning the factors jointly for the shared grid (equal work per workgroup, the trunk products filling the 512
  // workgroup slots exactly once: 84 -> ~40 MB of slabs) was measured and is SLOWER: 141 us + 14 us reduce against
  // 131.5 + 18.5 (`tools/scratch`-style sweep over slot targets 256..2048): uneven k-chunks lose the
  // per-problem XCD grouping and long workgroups run below the k-loop's steady rate.
  // env_mlp: the factors of every layer first (lx_env moves the first layer's), then ONE pass lays the slab out
  for (int l = 0; l < p->npl; ++l) {
    int sk = choose_splitk(p->pu[l], env_in(*p, l), p->mb, 1);
    // the first env layer's weight gradient is a launch of its own and has to fill the chip; the later ones share the
    // env-level launch with two other products: half the split (8 k-tiles per workgroup instead of 4, half the slab) --
    // env level 44.3 -> 42.4 us, slab sum 17.2 -> 15.4 us (every other factor: slower)
    if (l > 0 && sk > 1) sk /= 2;
    p->sk_env[l] = sk;
    // layer l's weight gradient and the data gradient into layer l - 1 as one row-block kernel (the last layer's
    // backward is k_latent_bwd's when lat_fused): decided from the shapes alone, like every other plan entry
    if (l >= 1 && l < p->npl - p->lat_fused - (p->ct_P > 0) && rb_level_shape_ok(p->mb, p->pu[l], p->pu[l - 1], 1)) {
      p->rb_env[l] = rb_level_ranges(p->mb, p->pu[l - 1], 1);
      p->sk_env[l] = p->rb_env[l];
    }
  }
  if (p->npl >= 2 && p->rb_env[1] && p->priv == 64) {
    // env layer 0's weight gradient from the data-gradient tiles of the level above: rb_env[1] partial records
    p->lx_env = 1;
    p->sk_env[0] = p->rb_env[1];
  }
  long long s = 0;
  for (int l = 0; l < p->npl; ++l) {
    p->s_envW[l] = s; s += (long long)p->sk_env[l] * p->pu[l] * env_in(*p, l);
    p->s_envB[l] = s; s += (long long)p->sk_env[l] * p->pu[l];
    s = (s + 3) & ~3LL;
  }
  {
    const int latz_on = latz_fuse_ref();
    // shapes only: the fused latent path with the row dots from the dZ1 tiles, the env level as the row-block kernel with the
    // first env layer's weight gradient in it, the reference's 128-wide second env layer
    p->latz = (latz_on && p->nets == 2 && p->lat_fused && p->npl == 3 && p->rb_env[1] && p->lx_env && p->pu[1] == 128 && p->lat_tiles <= 8 &&
               p->lat_blocks >= p->rb_env[1]) ? 1 : 0;
  }
  for (int l = 0; l < p->nl; ++l) {
    const int inw = (l == 0) ? p->xld : ac_in(*p, l);  // layer 0 multiplies the padded xcat
    p->sk_ac[l] = choose_splitk(p->u[l], inw, p->mb, p->nets);
    // (l >= 2: the data gradient into trunk layer 0 keeps its interleaved layout and the latent row dots)
    if (l >= 2 && rb_level_shape_ok(p->mb, p->u[l], p->u[l - 1], p->nets)) {
      p->rb_ac[l] = rb_level_ranges(p->mb, p->u[l - 1], p->nets);
      p->sk_ac[l] = p->rb_ac[l];
    }
    if (l == 0) {
      const int mt128 = p->mb / DMA_BM;
      const int chain = (mt128 % 4 == 0) ? 4 : ((mt128 % 2 == 0) ? 2 : 1);
      // shapes only (the launch re-checks pointers): row dots from those tiles, 32-wide padded input with a FREE last
      // column (xw <= 31: column 31 carries the ONE of the bias gradient; obs + latent == 32 takes the separate
      // weight-gradient launch), whole 128-row / 128-column tiles, the level-fused grid; two nets (the rider's partial
      // records and row dots are laid out per net pair: a shared trunk takes the separate weight-gradient launch)
      if (p->nets == 2 && p->nl >= 2 && p->lat_fused && p->xld == 32 && p->xw < 32 && (p->mb % DMA_BM) == 0 && (p->u[0] % 128) == 0 &&
          !bf16_mode() && p->mb >= 4) {
        p->lw_chain = chain;
        p->lw_parts = mt128 / chain;
        p->sk_ac[0] = p->lw_parts;
      }
    }
    // layout [split][net][...]: split stride = nets*size so the batch stride stays the net size
    p->s_acW[l] = s; s += (long long)p->sk_ac[l] * p->nets * p->u[l] * inw;
    p->s_acB[l] = s; s += (long long)p->sk_ac[l] * p->nets * p->u[l];
    s = (s + 3) & ~3LL;
  }
  p->slab_floats = s;
  p->w_slab = take(sizeof(float) * (size_t)s);
  p->w_sumsq = take(sizeof(double) * 2 * SUMSQ_BLOCKS);
  p->w_scal = take(sizeof(float) * 8);
  p->w_total = w;
  return 0;
}

template <typename T>
static inline T* wsp(const igi_teacher_state* st, size_t off) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(st->workspace) + off);
}

// ---------------------------------------------------------------------------------------------
// block reduction helpers (deterministic: fixed shuffle tree + fixed wave order)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// fp32 wave-wide sum, result in every lane.  DPP lane permutes inside each 16-lane row
// (quad_perm xor-1 / xor-2, row_half_mirror, row_mirror: 4 VALU ops, no LDS crossbar) and four
// v_readlane across the rows, instead of six dependent ds_bpermute round trips.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror  -> every lane of a row holds the row's sum
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}

// ---------------------------------------------------------------------------------------------
// 1. GAE + returns (experience.py:242-255): one thread per env walks T backwards over
//    [t][env]-coalesced loads.  Also accumulates the six fp64 sums that the advantage
//    normalisation (experience.py:261-262) and the two value_mean_std updates
//    (frozen_ppo.py:719-723) need.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void k_gae(const float* __restrict__ rewards,
                                                       const float* __restrict__ values,
                                                       const uint8_t* __restrict__ dones,
                                                       const float* __restrict__ last_values,
                                                       float* __restrict__ returns_raw, int N, int T,
                                                       float gamma, float gamma_tau,
                                                       double* __restrict__ partials) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  double s[6] = {0, 0, 0, 0, 0, 0};
  if (n < N) {
    float lam = 0.f;
    float nextv = last_values[n];
    for (int t = T - 1; t >= 0; --t) {
      const long long i = (long long)t * N + n;
      const float v = values[i];
      const float nn = 1.0f - (float)dones[i];
      // rewards + gamma*next_values*nn - values, each product/sum rounded (no contraction)
      const float delta = (rewards[i] + (gamma * nextv) * nn) - v;
      lam = delta + (gamma_tau * nn) * lam;
      const float ret = lam + v;
      returns_raw[i] = ret;
      const float adv = ret - v;
      s[0] += adv; s[1] += (double)adv * adv;
      s[2] += v;   s[3] += (double)v * v;
      s[4] += ret; s[5] += (double)ret * ret;
      nextv = v;
    }
  }
  __shared__ double red[PREP_THREADS / 64][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double r = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = r;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double r = 0;
    for (int w = 0; w < PREP_THREADS / 64; ++w) r += red[w][threadIdx.x];
    partials[blockIdx.x * 6 + threadIdx.x] = r;
  }
}

__device__ __forceinline__ void chan_merge(double& mean, double& var, double& count, float b_mean,
                                           float b_var, double n) {
  // running_mean_std.py:48-58 with fp32 batch moments promoted to fp64
  const double delta = (double)b_mean - mean;
  const double tot = count + n;
  const double new_mean = mean + delta * n / tot;
  const double m2 = var * count + (double)b_var * n + delta * delta * count * n / tot;
  mean = new_mean;
  var = m2 / tot;
  count = tot;
}

// coef: [adv_mean, adv_std+1e-8, v_mean, v_den, r_mean, r_den]
__global__ void k_prep_final(const double* __restrict__ partials, int nblocks, long long B,
                             double* __restrict__ rms_value, float eps, float* __restrict__ coef,
                             int normalize_value) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nblocks; ++b)
    for (int j = 0; j < 6; ++j) s[j] += partials[b * 6 + j];
  const double n = (double)B;
  float mean[3], var[3];
  for (int q = 0; q < 3; ++q) {
    const double m = s[2 * q] / n;
    double v = (s[2 * q + 1] - n * m * m) / (n - 1.0);  // unbiased (torch.std / var default)
    if (v < 0) v = 0;
    mean[q] = (float)m;
    var[q] = (float)v;
  }
  coef[0] = mean[0];
  coef[1] = sqrtf(var[0]) + 1e-8f;
  if (!normalize_value) return;
  double rm = rms_value[0], rv = rms_value[1], rc = rms_value[2];
  chan_merge(rm, rv, rc, mean[1], var[1], n);       // value_mean_std(values)  (train)
  coef[2] = (float)rm;
  coef[3] = sqrtf((float)rv + eps);
  chan_merge(rm, rv, rc, mean[2], var[2], n);       // value_mean_std(returns) (train)
  coef[4] = (float)rm;
  coef[5] = sqrtf((float)rv + eps);
  rms_value[0] = rm; rms_value[1] = rv; rms_value[2] = rc;
}

__device__ __forceinline__ float clamp5(float y) { return fminf(fmaxf(y, -5.0f), 5.0f); }

__global__ __launch_bounds__(PREP_THREADS) void k_prep_norm(
    const float* __restrict__ values, const float* __restrict__ returns_raw,
    const float* __restrict__ mus, const float* __restrict__ sigmas, const float* __restrict__ coef,
    float* __restrict__ adv, float* __restrict__ values_n, float* __restrict__ returns_n,
    float* __restrict__ mus_w, float* __restrict__ sigmas_w, long long B, int act,
    int normalize_value) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float am = coef[0], ad = coef[1], vm = coef[2], vd = coef[3], rm = coef[4], rd = coef[5];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
    const float v = values[i], r = returns_raw[i];
    adv[i] = ((r - v) - am) / ad;
    values_n[i] = normalize_value ? clamp5((v - vm) / vd) : v;
    returns_n[i] = normalize_value ? clamp5((r - rm) / rd) : r;
  }
  const long long BA = B * act;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < BA; i += stride) {
    mus_w[i] = mus[i];
    sigmas_w[i] = sigmas[i];
  }
}

// ---------------------------------------------------------------------------------------------
// 2. minibatch gather (experience.py:207-226) + column statistics for the two in-loop
//    RunningMeanStd updates (frozen_ppo.py:521-522).  Each block stages gs_rows gathered rows in
//    LDS, writes them out raw, then one thread per column sums that tile in fp64.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_THREADS) void k_gather_stats(
    const float* __restrict__ obses, const float* __restrict__ priv_info,
    const int64_t* __restrict__ perm, long long start, int mb, int N, int T, int obs, int priv,
    int rows_per_block, float* __restrict__ xcat, int xld, float* __restrict__ priv_g, int pld,
    double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int D = obs + priv;
  const int LD = D + 1;
  const int r0 = blockIdx.x * rows_per_block;
  const int nrows = min(rows_per_block, mb - r0);
  int* rowi = reinterpret_cast<int*>(tile + rows_per_block * LD);  // time-major element index per row
  for (int r = threadIdx.x; r < nrows; r += blockDim.x) {
    const long long b = perm[start + r0 + r];
    const int n = (int)(b / T);
    rowi[r] = (int)(b - (long long)n * T) * N + n;   // b = n*T + t  ->  t*N + n
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nrows * obs; e += blockDim.x) {
    const int r = e / obs, c = e - r * obs;
    const float x = obses[(long long)rowi[r] * obs + c];
    tile[r * LD + c] = x;
    xcat[(long long)(r0 + r) * xld + c] = x;
  }
  for (int e = threadIdx.x; e < nrows * priv; e += blockDim.x) {
    const int r = e / priv, c = e - r * priv;
    const float x = priv_info[(long long)rowi[r] * priv + c];
    tile[r * LD + obs + c] = x;
    priv_g[(long long)(r0 + r) * pld + c] = x;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    double s = 0, s2 = 0;
    for (int r = 0; r < nrows; ++r) {
      const double x = tile[r * LD + c];
      s += x;
      s2 += x * x;
    }
    partials[((long long)blockIdx.x * D + c) * 2 + 0] = s;
    partials[((long long)blockIdx.x * D + c) * 2 + 1] = s2;
  }
}

// one block of 1024 threads: thread (c = tid % 128, j = tid / 128) sums the per-block partials
// b = j, j+8, ... of column c in fixed order; 8 sub-sums are then combined in fixed order, merged
// into the fp64 running state and the fp32 (mean, sqrt(var+eps)) pair of the normalise pass emitted.
constexpr int RMSF_THREADS = 1024;
__global__ __launch_bounds__(RMSF_THREADS) void k_rms_final(const double* __restrict__ partials,
                                                             int nblocks, int rows, int obs, int priv,
                                                             double* __restrict__ rms_obs,
                                                             double* __restrict__ rms_priv, float eps,
                                                             float* __restrict__ coef) {
  const int D = obs + priv;
  __shared__ double sh[2][8][128];
  __shared__ double cnt[2];
  if (threadIdx.x == 0) { cnt[0] = rms_obs[2 * obs]; cnt[1] = rms_priv[2 * priv]; }
  const double n = (double)rows;
  const int cl = threadIdx.x & 127, j = threadIdx.x >> 7;
  for (int c0 = 0; c0 < D; c0 += 128) {
    const int c = c0 + cl;
    double s = 0, s2 = 0;
    if (c < D) {
      for (int b = j; b < nblocks; b += 8) {
        s += partials[((long long)b * D + c) * 2 + 0];
        s2 += partials[((long long)b * D + c) * 2 + 1];
      }
    }
    sh[0][j][cl] = s;
    sh[1][j][cl] = s2;
    __syncthreads();
    if (j == 0 && c < D) {
      s = 0; s2 = 0;
      for (int q = 0; q < 8; ++q) { s += sh[0][q][cl]; s2 += sh[1][q][cl]; }
      const double m = s / n;
      double v = (s2 - n * m * m) / (n - 1.0);
      if (v < 0) v = 0;
      const bool is_obs = c < obs;
      double* stt = is_obs ? rms_obs : rms_priv;
      const int d = is_obs ? obs : priv;
      const int cc = is_obs ? c : c - obs;
      double mean = stt[cc], var = stt[d + cc], count = cnt[is_obs ? 0 : 1];
      chan_merge(mean, var, count, (float)m, (float)v, n);
      stt[cc] = mean;
      stt[d + cc] = var;
      coef[2 * c + 0] = (float)mean;
      coef[2 * c + 1] = sqrtf((float)var + eps);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { rms_obs[2 * obs] = cnt[0] + n; rms_priv[2 * priv] = cnt[1] + n; }
}

// eval-mode coefficients straight from the running state (model_act path)
__global__ void k_rms_coef(int obs, int priv, const double* __restrict__ rms_obs,
                           const double* __restrict__ rms_priv, float eps, float* __restrict__ coef) {
  const int D = obs + priv;
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    const bool is_obs = c < obs;
    const double* stt = is_obs ? rms_obs : rms_priv;
    const int d = is_obs ? obs : priv;
    const int cc = is_obs ? c : c - obs;
    coef[2 * c + 0] = (float)stt[cc];
    coef[2 * c + 1] = sqrtf((float)stt[d + cc] + eps);
  }
}

// ---- normaliser trajectory ---------------------------------------------------------------------
// The two in-loop RunningMeanStd updates (frozen_ppo.py:521-522) depend only on the rollout and the
// fixed permutation, never on the parameters: minibatch i has the same batch moments in every
// mini-epoch.  So the whole sequence of E*n_mb Chan merges is evaluated ONCE per update (8 moment
// reductions + one 79-thread scan) and every optimizer step just looks its (mean, sqrt(var+eps)) up:
// the per-step critical path loses a grid-wide reduction and two launches.
__global__ __launch_bounds__(RMSF_THREADS) void k_mb_moments(const double* __restrict__ partials, int nblocks,
                                                             int rows, int D, float* __restrict__ moments) {
  __shared__ double sh[2][8][128];
  const double* part = partials + (long long)blockIdx.x * nblocks * D * 2;
  float* mom = moments + (long long)blockIdx.x * D * 2;
  const double n = (double)rows;
  const int cl = threadIdx.x & 127, j = threadIdx.x >> 7;
  for (int c0 = 0; c0 < D; c0 += 128) {
    const int c = c0 + cl;
    double s = 0, s2 = 0;
    if (c < D) {
      for (int b = j; b < nblocks; b += 8) {
        s += part[((long long)b * D + c) * 2 + 0];
        s2 += part[((long long)b * D + c) * 2 + 1];
      }
    }
    sh[0][j][cl] = s;
    sh[1][j][cl] = s2;
    __syncthreads();
    if (j == 0 && c < D) {
      s = 0; s2 = 0;
      for (int q = 0; q < 8; ++q) { s += sh[0][q][cl]; s2 += sh[1][q][cl]; }
      const double m = s / n;
      double v = (s2 - n * m * m) / (n - 1.0);
      if (v < 0) v = 0;
      mom[2 * c] = (float)m;       // fp32 batch moments, as x.mean(0) / x.var(0) are
      mom[2 * c + 1] = (float)v;
    }
    __syncthreads();
  }
}

// thread c scans column c through all steps; state row layout: [obs mean, obs var, obs count | priv ...]
__global__ void k_rms_traj(const float* __restrict__ moments, int nmb, int steps, int rows, int obs, int priv,
                           const double* __restrict__ rms_obs, const double* __restrict__ rms_priv, float eps,
                           float* __restrict__ traj_coef, double* __restrict__ traj_state) {
  const int D = obs + priv;
  const int srow = 2 * D + 2;
  const double n = (double)rows;
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    const bool is_obs = c < obs;
    const double* stt = is_obs ? rms_obs : rms_priv;
    const int d = is_obs ? obs : priv;
    const int cc = is_obs ? c : c - obs;
    const int base = is_obs ? 0 : 2 * obs + 1;
    double mean = stt[cc], var = stt[d + cc], count = stt[2 * d];
    for (int k = 0; k < steps; ++k) {
      const float* mom = moments + ((long long)(k % nmb) * D + c) * 2;
      chan_merge(mean, var, count, mom[0], mom[1], n);
      traj_coef[((long long)k * D + c) * 2] = (float)mean;
      traj_coef[((long long)k * D + c) * 2 + 1] = sqrtf((float)var + eps);
      double* row = traj_state + (long long)k * srow + base;
      row[cc] = mean;
      row[d + cc] = var;
      if (cc == 0) row[2 * d] = count;
    }
  }
}

// per step: gather the minibatch rows, normalise with the step's looked-up statistics, publish the
// step's running state, and refresh the zero-padded first-layer weight (extra blocks).
struct GatherArgs {
  const float* obses; const float* priv_info; const int64_t* perm;
  long long start; int mb, N, T, obs, priv, rows_per_block, gather_blocks;
  const float* coef; const double* state_row; double* rms_obs; double* rms_priv;
  float* xcat; int xld, xw; float* priv_g; int pld;
  const float* params; long long o_w, ac_block; int u0, u0p; float* w1p; float* wlat; int K2p;
  int nets = 2;                    // trunks mirrored in w1p / wlat
  const int32_t* stop = nullptr;   // KL early stopping: the stop word; >= 0 = the update has stopped, this body is inert
};

// bid / nblocks: this body's block index and block count (it also runs as the second half of k_adam_gather)
__device__ __forceinline__ void gather_normalize_body(const GatherArgs& a, int bid, int nblocks) {
  const float* __restrict__ obses = a.obses; const float* __restrict__ priv_info = a.priv_info;
  const int64_t* __restrict__ perm = a.perm;
  const long long start = a.start; const int mb = a.mb, N = a.N, T = a.T, obs = a.obs, priv = a.priv;
  const int rows_per_block = a.rows_per_block, gather_blocks = a.gather_blocks;
  const float* __restrict__ coef = a.coef; const double* __restrict__ state_row = a.state_row;
  double* __restrict__ rms_obs = a.rms_obs; double* __restrict__ rms_priv = a.rms_priv;
  float* __restrict__ xcat = a.xcat; const int xld = a.xld, xw = a.xw; float* __restrict__ priv_g = a.priv_g;
  const int pld = a.pld; const float* __restrict__ params = a.params; const long long o_w = a.o_w, ac_block = a.ac_block;
  const int u0 = a.u0, u0p = a.u0p; float* __restrict__ w1p = a.w1p; float* __restrict__ wlat = a.wlat;
  const int K2p = a.K2p;
  if (a.stop && a.stop[0] >= 0) return;   // stopped: neither the next step's running state nor its rows (block-uniform)
  if (bid >= gather_blocks) {  // W1p[net][o][c] refresh (see k_pad_w1)
    const int total = a.nets * u0p * xld;
    const int nb = nblocks - gather_blocks;
    for (int e = (bid - gather_blocks) * blockDim.x + threadIdx.x; e < total; e += nb * blockDim.x) {
      const int c = e % xld;
      const int o = (e / xld) % u0p;
      const int net = e / (xld * u0p);
      const float v = (c < xw && o < u0) ? params[o_w + net * ac_block + (long long)o * xw + c] : 0.f;
      w1p[e] = v;
      // compact, transposed copy of the 8 latent columns for k_latent_bwd: wlat[j][k], k = net*u0p + o
      if (wlat && c >= obs && c < obs + 8) wlat[(long long)(c - obs) * K2p + net * u0p + o] = v;
    }
    if (wlat) {  // zero tail k in [nets*u0p, K2p)
      const int tail = K2p - a.nets * u0p;
      for (int e = (bid - gather_blocks) * blockDim.x + threadIdx.x; e < 8 * tail; e += nb * blockDim.x)
        wlat[(long long)(e / tail) * K2p + a.nets * u0p + e % tail] = 0.f;
    }
    return;
  }
  __shared__ int rowi[64];
  if (bid == 0) {  // the running state after this step (what RunningMeanStd would now hold)
    for (int e = threadIdx.x; e < 2 * obs + 1; e += blockDim.x) rms_obs[e] = state_row[e];
    for (int e = threadIdx.x; e < 2 * priv + 1; e += blockDim.x) rms_priv[e] = state_row[2 * obs + 1 + e];
  }
  const int r0 = bid * rows_per_block;
  const int nrows = min(rows_per_block, mb - r0);
  for (int r = threadIdx.x; r < nrows; r += blockDim.x) {
    const long long b = perm[start + r0 + r];
    const int n = (int)(b / T);
    rowi[r] = (int)(b - (long long)n * T) * N + n;
  }
  __syncthreads();
  // wave w takes rows w, w+4, ...; lanes stride the columns (no per-element integer division)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  // a wave's rows eight at a time: the eight gathered loads go out together (one per trip was eight dependent round
  // trips per wave -- the whole 12 us of this body)
  for (int c = lane; c < priv; c += 64) {
    const float m = coef[2 * (obs + c)], d = coef[2 * (obs + c) + 1];
    for (int rb = wave; rb < nrows; rb += 8 * nw) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = priv_info[(long long)rowi[min(rb + u * nw, nrows - 1)] * priv + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = rb + u * nw;
        if (r < nrows) priv_g[(long long)(r0 + r) * pld + c] = clamp5((x[u] - m) / d);
      }
    }
  }
  for (int c = lane; c < xld; c += 64) {
    if (c < obs) {
      const float m = coef[2 * c], d = coef[2 * c + 1];
      for (int rb = wave; rb < nrows; rb += 8 * nw) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = obses[(long long)rowi[min(rb + u * nw, nrows - 1)] * obs + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = rb + u * nw;
          if (r < nrows) xcat[(long long)(r0 + r) * xld + c] = clamp5((x[u] - m) / d);
        }
      }
    } else if (c >= xw) {
      for (int r = wave; r < nrows; r += nw) xcat[(long long)(r0 + r) * xld + c] = 0.f;  // keep the padding zero
    }
  }
}

__global__ __launch_bounds__(GS_THREADS) void k_gather_normalize(const GatherArgs a) {
  gather_normalize_body(a, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(256) void k_normalize(float* __restrict__ xcat, int xld, int xw,
                                                   float* __restrict__ priv_g, int pld, int rows,
                                                   int obs, int priv,
                                                   const float* __restrict__ coef) {
  const int D = obs + priv;
  const long long total = (long long)rows * D;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long r = e / D;
    const int c = (int)(e - r * D);
    const float m = coef[2 * c], d = coef[2 * c + 1];
    float* p = (c < obs) ? &xcat[r * xld + c] : &priv_g[r * pld + (c - obs)];
    *p = clamp5((*p - m) / d);
  }
  // keep the zero padding of xcat zero (columns xw..xld-1 feed the padded first layer)
  const int padw = xld - xw;
  const long long ptotal = (long long)rows * padw;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ptotal; e += stride) {
    const long long r = e / padw;
    xcat[r * xld + xw + (int)(e - r * padw)] = 0.f;
  }
}

// raw (un-gathered) rows -> workspace, for the inference path
__global__ __launch_bounds__(256) void k_copy_rows(const float* __restrict__ obs_in,
                                                   const float* __restrict__ priv_in, int rows, int obs,
                                                   int priv, float* __restrict__ xcat, int xld,
                                                   float* __restrict__ priv_g, int pld) {
  const int D = obs + priv;
  const long long total = (long long)rows * D;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long r = e / D;
    const int c = (int)(e - r * D);
    if (c < obs) xcat[r * xld + c] = obs_in[r * obs + c];
    else priv_g[r * pld + (c - obs)] = priv_in[r * priv + (c - obs)];
  }
}

// kernels templated on MAXJ, the number of 64-column groups of the last hidden layer (H columns) that a lane holds
#define IGI_LAUNCH_MAXJ(kernel, H, grid, block, shm, stream, ...)                        \
  do {                                                                                   \
    const int _maxj = ((H) + 63) / 64;                                                   \
    if (_maxj <= 1) IGI_LAUNCH(kernel<1>, grid, block, shm, stream, __VA_ARGS__);        \
    else if (_maxj == 2) IGI_LAUNCH(kernel<2>, grid, block, shm, stream, __VA_ARGS__);   \
    else IGI_LAUNCH(kernel<4>, grid, block, shm, stream, __VA_ARGS__);                   \
  } while (0)

// ---------------------------------------------------------------------------------------------
// 3. heads + PPO loss + head backward (models_split.py:222-250; frozen_ppo.py:543-570, 618): ppo_loss.h
// ---------------------------------------------------------------------------------------------
}  // namespace igi
#include "ppo_loss.h"
namespace igi {

// One wave per row: this lane's share of the head products of a row, the value's in pv and mu[q]'s in pm[q], q < act
// (plain multiply and add; a wave_sum of each completes it).  Shared by the inference and the rollout-step kernel so
// that both give the same bits.
template <int MAXJ>
__device__ __forceinline__ void head_products_row(const float* __restrict__ ha_p, const float* __restrict__ hc_p, int H,
                                                  const float* __restrict__ Wmu, const float* __restrict__ Wv, int act,
                                                  int lane, float (&pm)[IGI_MAX_ACT], float& pv) {
  pv = 0.f;
#pragma unroll
  for (int q = 0; q < IGI_MAX_ACT; ++q) pm[q] = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int k = lane + 64 * j;
    if (k < H) {
      const float ha = ha_p[k], hc = hc_p[k];
      pv += hc * Wv[k];
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q)
        if (q < act) pm[q] += ha * Wmu[q * H + k];
    }
  }
}

// inference heads: mu (rows,act), value (rows,1)
template <int MAXJ>
__global__ __launch_bounds__(256) void k_heads_infer(const float* __restrict__ h, long long net_stride,
                                                     int ldh, int H, const float* __restrict__ Wmu,
                                                     const float* __restrict__ bmu,
                                                     const float* __restrict__ Wv,
                                                     const float* __restrict__ bv, int rows, int act,
                                                     float* __restrict__ mu_out,
                                                     float* __restrict__ v_out) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nw = (gridDim.x * blockDim.x) >> 6;
  for (int row = gw; row < rows; row += nw) {
    const float* ha_p = h + (long long)row * ldh;
    float pm[IGI_MAX_ACT], pv;
    head_products_row<MAXJ>(ha_p, ha_p + net_stride, H, Wmu, Wv, act, lane, pm, pv);
    pv = wave_sum(pv);
#pragma unroll
    for (int q = 0; q < IGI_MAX_ACT; ++q)
      if (q < act) pm[q] = wave_sum(pm[q]);
    if (v_out && lane == 0) v_out[row] = pv + bv[0];
    if (mu_out) {
#pragma unroll
      for (int q = 0; q < IGI_MAX_ACT; ++q)
        if (q < act && lane == q) mu_out[(long long)row * act + q] = pm[q] + bmu[q];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 4. gradient assembly: fixed-order sum of the split-K slabs / per-block head partials into the
//    flat gradient vector (bitwise reproducible: no atomics anywhere on the path).
// ---------------------------------------------------------------------------------------------
struct Segment {
  long long dst;      // offset in the flat gradient
  const float* src;   // first partial
  long long stride;   // between partials
  int count;          // elements = rows * cols
  int cols, src_ld;   // element e lives at (e / cols) * src_ld + e % cols of a partial (src_ld 0: dense)
  int nparts;
};
struct SegTable {
  Segment s[MAX_SEG];
  int n;
  int wide = 0;   // 1: dense 16-byte-aligned segments with >= 64 partials take the 16-byte part-group path (the student's
                  // per-workgroup gradient records: 170 - 512 partials of 16 - 80 K floats)
};

// KL early stopping as the statistics block sees it: state == NULL = off.  slot: this optimizer step; limit = 1.5 *
// kl_threshold.  state[0] the stop word (int32; -1 = running), state[2 + s] approx_kl of step s (float bits).
// exchange != 0 (data parallel): the block stores this rank's estimator in the exchange scratch, state[1], and leaves
// the word alone -- k_stop_decide writes it from the rank sum.
struct StopArgs { int32_t* state; int slot; double limit; int exchange; };

// strided fixed-order sums of the loss partial records -> the statistics row (means over the minibatch); one block.
// With early stopping it also takes the step's decision (frozen_ppo.py:578-581): thread 5, which holds the approx_kl
// column, stores the estimator and the stop word -- plain stores, ahead of the Adam launch in stream order.  Step 0
// decides whatever the word held (the previous update's result); a later step of a stopped update writes nothing.
__device__ __forceinline__ void stats_row_block(const double* __restrict__ loss_part, int loss_blocks, int mb,
                                                float* __restrict__ stats_row, const StopArgs stop = StopArgs{nullptr, 0, 0.0, 0}) {
  const bool live = !stop.state || stop.slot == 0 || stop.state[0] < 0;   // read before the barrier, written behind it
  // thread (q = tid&7, j = tid>>3): strided fixed-order partial sums, then a fixed tree in LDS
  __shared__ double sh[256];
  const int q = threadIdx.x & 7, j = threadIdx.x >> 3;
  double s = 0;
  for (int b0 = j; b0 < loss_blocks; b0 += 32 * 8) {  // 8 independent loads in flight, fixed order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = b0 + 32 * u;
      v[u] = (b < loss_blocks) ? loss_part[b * 8 + q] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < 5 && live) {
    double t = 0;
    for (int jj = 0; jj < 32; ++jj) t += sh[jj * 8 + threadIdx.x];
    stats_row[threadIdx.x] = (float)(t / (double)mb);
  }
  if (threadIdx.x == 5 && stop.state && live) {
    double t = 0;
    for (int jj = 0; jj < 32; ++jj) t += sh[jj * 8 + 5];
    const float akl = (float)(t / (double)mb);
    reinterpret_cast<float*>(stop.state)[2 + stop.slot] = akl;
    if (stop.exchange) reinterpret_cast<float*>(stop.state)[1] = akl;
    else stop.state[0] = ((double)akl > stop.limit) ? stop.slot : -1;
  }
}

constexpr int SLAB_GX = 256;
// grid (SLAB_GX, segments).  A block covers 256/G consecutive elements with G part-groups: thread
// (e = tid % (256/G), grp = tid / (256/G)) sums parts grp, grp+G, ... with 4 independent
// accumulators; groups are combined through LDS in fixed order.  G grows with the number of
// partials so long part lists (per-block head partials) are not a serial chain.
__global__ __launch_bounds__(RED_THREADS) void k_slab_reduce(const SegTable t, float* __restrict__ grads) {
  __shared__ float sh[RED_THREADS];
  const Segment sg = t.s[blockIdx.y];
  // 16-byte path (dense, aligned segments with few partials = the big split-K slabs): four elements per
  // thread and part, four parts in flight -> 16x the bytes in flight of the scalar path below
  if (sg.src_ld == 0 && sg.nparts < 64 && (sg.count & 3) == 0 && (sg.stride & 3) == 0 && (sg.dst & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(sg.src) & 15) == 0 && (reinterpret_cast<uintptr_t>(grads) & 15) == 0) {
    const int n4 = sg.count >> 2;
    for (int e = blockIdx.x * RED_THREADS + threadIdx.x; e < n4; e += gridDim.x * RED_THREADS) {
      const float4* p = reinterpret_cast<const float4*>(sg.src) + e;
      const long long st4 = sg.stride >> 2;
      float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
      int k = 0;
      for (; k + 3 < sg.nparts; k += 4) {
        const float4 a0 = p[k * st4], a1 = p[(k + 1) * st4], a2 = p[(k + 2) * st4], a3 = p[(k + 3) * st4];
        s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
        s1.x += a1.x; s1.y += a1.y; s1.z += a1.z; s1.w += a1.w;
        s2.x += a2.x; s2.y += a2.y; s2.z += a2.z; s2.w += a2.w;
        s3.x += a3.x; s3.y += a3.y; s3.z += a3.z; s3.w += a3.w;
      }
      for (; k < sg.nparts; ++k) {
        const float4 a0 = p[k * st4];
        s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
      }
      float4 o;
      o.x = (s0.x + s1.x) + (s2.x + s3.x); o.y = (s0.y + s1.y) + (s2.y + s3.y);
      o.z = (s0.z + s1.z) + (s2.z + s3.z); o.w = (s0.w + s1.w) + (s2.w + s3.w);
      *reinterpret_cast<float4*>(grads + sg.dst + 4 * (long long)e) = o;
    }
    return;
  }
  if (t.wide && sg.src_ld == 0 && sg.nparts >= 64 && (sg.count & 3) == 0 && (sg.stride & 3) == 0 && (sg.dst & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(sg.src) & 15) == 0 && (reinterpret_cast<uintptr_t>(grads) & 15) == 0) {
    // many partials of a wide record: a block covers 64 consecutive elements (16 lanes x 16 bytes: 256 contiguous bytes
    // per partial) with 16 part-groups; group g sums partials g, g + 16, ... with four independent accumulators, the
    // groups meet in LDS in fixed order.  (The scalar path below gave every group 8 elements = 32 bytes per partial.)
    __shared__ float4 sh4[RED_THREADS];
    const int e4l = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int n4 = sg.count >> 2;
    const long long st4 = sg.stride >> 2;
    for (int b0 = blockIdx.x * 16; b0 < n4; b0 += gridDim.x * 16) {
      const int e = b0 + e4l;
      float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
      if (e < n4) {
        const float4* p = reinterpret_cast<const float4*>(sg.src) + e;
        int k = grp;
        for (; k + 48 < sg.nparts; k += 64) {
          const float4 a0 = p[k * st4], a1 = p[(k + 16) * st4], a2 = p[(k + 32) * st4], a3 = p[(k + 48) * st4];
          s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
          s1.x += a1.x; s1.y += a1.y; s1.z += a1.z; s1.w += a1.w;
          s2.x += a2.x; s2.y += a2.y; s2.z += a2.z; s2.w += a2.w;
          s3.x += a3.x; s3.y += a3.y; s3.z += a3.z; s3.w += a3.w;
        }
        for (; k < sg.nparts; k += 16) {
          const float4 a0 = p[k * st4];
          s0.x += a0.x; s0.y += a0.y; s0.z += a0.z; s0.w += a0.w;
        }
      }
      float4 o;
      o.x = (s0.x + s1.x) + (s2.x + s3.x); o.y = (s0.y + s1.y) + (s2.y + s3.y);
      o.z = (s0.z + s1.z) + (s2.z + s3.z); o.w = (s0.w + s1.w) + (s2.w + s3.w);
      sh4[threadIdx.x] = o;
      __syncthreads();
      if (grp == 0 && e < n4) {
        float4 v = sh4[e4l];
#pragma unroll
        for (int q = 1; q < 16; ++q) {
          const float4 u = sh4[q * 16 + e4l];
          v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        *reinterpret_cast<float4*>(grads + sg.dst + 4 * (long long)e) = v;
      }
      __syncthreads();
    }
    return;
  }
  const int G = sg.nparts >= 256 ? 32 : (sg.nparts >= 64 ? 8 : 1);
  const int epb = RED_THREADS / G;
  const int el = threadIdx.x % epb, grp = threadIdx.x / epb;
  for (int e0 = blockIdx.x * epb; e0 < sg.count; e0 += gridDim.x * epb) {
    const int e = e0 + el;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (e < sg.count) {
      const long long off = sg.src_ld ? (long long)(e / sg.cols) * sg.src_ld + (e % sg.cols) : e;
      const float* p = sg.src + off;
      const long long st = sg.stride * G;
      int k = grp;
      for (; k + 3 * G < sg.nparts; k += 4 * G) {
        const float* q = p + (long long)k * sg.stride;
        s0 += q[0]; s1 += q[st]; s2 += q[2 * st]; s3 += q[3 * st];
      }
      for (; k < sg.nparts; k += G) s0 += p[(long long)k * sg.stride];
    }
    float v = (s0 + s1) + (s2 + s3);
    if (G > 1) {
      sh[threadIdx.x] = v;
      __syncthreads();
      if (grp == 0) {
        v = 0.f;
        for (int q = 0; q < G; ++q) v += sh[q * epb + el];
      }
      __syncthreads();
    }
    if (grp == 0 && e < sg.count) grads[sg.dst + e] = v;
  }
}

// sum of squares of (grad*scale) and of the parameters, per block, in fp64; the extra last block
// turns the loss partials into the stats row (means over the minibatch).
__global__ __launch_bounds__(256) void k_sumsq_stats(const float* __restrict__ grads,
                                                     const float* __restrict__ params, long long P,
                                                     float scale, double* __restrict__ part,
                                                     const double* __restrict__ loss_part,
                                                     int loss_blocks, int mb,
                                                     float* __restrict__ stats_row,
                                                     const StopArgs stop = StopArgs{nullptr, 0, 0.0, 0}) {
  __shared__ double red[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == SUMSQ_BLOCKS) {
    stats_row_block(loss_part, loss_blocks, mb, stats_row, stop);
    return;
  }
  double sg = 0, sp = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < P;
       i += (long long)SUMSQ_BLOCKS * blockDim.x) {
    const double g = (double)(grads[i] * scale);
    const double p = (double)params[i];
    sg += g * g;
    sp += p * p;
  }
  sg = wave_sum(sg);
  sp = wave_sum(sp);
  if (lane == 0) { red[0][wave] = sg; red[1][wave] = sp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2 + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[blockIdx.x * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// clip_grad_norm_ + torch.optim.Adam single-tensor step (frozen_ppo.py:608-610).
// Where the parameters of the first trunk layer sit and where their zero-padded / transposed working copies go
// (see k_pad_w1 and the extra blocks of k_gather_normalize): the fused tail keeps those copies current from inside
// the Adam pass, so the next step needs no refresh launch.
struct W1Mirror {
  float* w1p; float* wlat;
  long long o_w, ac_block; int u0, u0p, xw, xld, obs, K2p;
  int nets;   // 1: no critic block behind the actor's (what follows it are the heads: never mirrored)
};

__device__ __forceinline__ void clip_adam_body(float* __restrict__ params, const float* __restrict__ grads,
                                               float* __restrict__ m, float* __restrict__ v, long long P,
                                               const double* __restrict__ part, float scale, float max_norm, float w1,
                                               float beta2, float w2, float step_size, float bc2_sqrt, float eps,
                                               float* __restrict__ stats_row, float decay, float l2, int bid,
                                               int nblocks, const W1Mirror* mir, const double* __restrict__ lr_dev = nullptr,
                                               double bc1 = 1.0, const int32_t* stop = nullptr) {
  // KL early stopping: this step's decision (or an earlier one) stopped the update -> parameters, moments, the
  // first-layer copies and slots 5 .. 7 of the row stay as step s - 1 left them (block-uniform, ahead of any barrier)
  if (stop && stop[0] >= 0) return;
  __shared__ float s_coef;
  __shared__ float s_step;
  __shared__ double s_part[2][64];
  if (threadIdx.x < 64) {
    // 128 partial pairs: lane b of the first wave adds pairs b and b + 64, lane 0 finishes in lane order
    // (every block repeats this, so a serial chain of 256 loads sat in front of each block's real work)
    double sg = 0, sp = 0;
#pragma unroll 2
    for (int b = threadIdx.x; b < SUMSQ_BLOCKS; b += 64) { sg += part[2 * b]; sp += part[2 * b + 1]; }
    s_part[0][threadIdx.x] = sg;
    s_part[1][threadIdx.x] = sp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sg = 0, sp = 0;
#pragma unroll 4
    for (int b = 0; b < 64; ++b) { sg += s_part[0][b]; sp += s_part[1][b]; }
    const float total = (float)sqrt(sg);
    float coef = 1.0f;
    if (max_norm > 0.f) coef = fminf(max_norm / (total + 1e-6f), 1.0f);
    s_coef = coef;
    if (bid == 0 && stats_row) {
      stats_row[5] = total;
      stats_row[6] = (float)sqrt(sp);  // the reference logs the PARAMETER norm as "grad_norms"
      stats_row[7] = coef;
    }
    if (lr_dev) {
      // adaptive schedule: the rate is a device double; the step size is the host line's arithmetic, (float)(lr / bc1)
      const double lr = *lr_dev;
      s_step = (float)(lr / bc1);
      if (bid == 0 && stats_row) stats_row[7] = (float)lr;   // the rate this step used (replaces the clip coefficient)
    }
  }
  __syncthreads();
  const float coef = s_coef;
  if (lr_dev) step_size = s_step;
  // one element: exactly torch's single-tensor Adam arithmetic (each line one rounding, -ffp-contract=off)
  auto one = [&](long long i, float gi, float& pi, float& mi, float& vi) {
    float g = (gi * scale) * coef;
    if (l2 != 0.f) g += l2 * pi;        // torch.optim.Adam(weight_decay=...): L2 term joins the clipped gradient
    mi = mi + w1 * (g - mi);            // exp_avg.lerp_(grad, 1-beta1)
    vi = vi * beta2 + (w2 * g) * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    // AdamW: param.mul_(1 - lr * weight_decay) first (decay == 1 for plain Adam: exact no-op)
    pi = pi * decay + (-step_size) * (mi / denom);  // param.addcdiv_(exp_avg, denom, -step_size)
    if (mir) {  // W1p[net][o][c] and the transposed latent columns follow the parameter they copy
      long long rel = i - mir->o_w;
      int net = 0;
      if (mir->nets == 2 && rel >= mir->ac_block) { rel -= mir->ac_block; net = 1; }
      if (rel >= 0 && rel < (long long)mir->u0 * mir->xw) {
        const int o = (int)(rel / mir->xw), c = (int)(rel - (long long)o * mir->xw);
        mir->w1p[((long long)net * mir->u0p + o) * mir->xld + c] = pi;
        if (mir->wlat && c >= mir->obs && c < mir->obs + 8)
          mir->wlat[(long long)(c - mir->obs) * mir->K2p + net * mir->u0p + o] = pi;
      }
    }
  };
  const bool vec = (P & 3) == 0 && ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) |
                                     reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  if (vec) {  // 16-byte accesses: four consecutive elements per thread and trip
    const long long P4 = P >> 2;
#pragma unroll 1
    for (long long q = (long long)bid * blockDim.x + threadIdx.x; q < P4; q += (long long)nblocks * blockDim.x) {
      const float4 g4 = reinterpret_cast<const float4*>(grads)[q];
      float4 p4 = reinterpret_cast<float4*>(params)[q];
      float4 m4 = reinterpret_cast<float4*>(m)[q], v4 = reinterpret_cast<float4*>(v)[q];
      one(4 * q + 0, g4.x, p4.x, m4.x, v4.x);
      one(4 * q + 1, g4.y, p4.y, m4.y, v4.y);
      one(4 * q + 2, g4.z, p4.z, m4.z, v4.z);
      one(4 * q + 3, g4.w, p4.w, m4.w, v4.w);
      reinterpret_cast<float4*>(params)[q] = p4;
      reinterpret_cast<float4*>(m)[q] = m4;
      reinterpret_cast<float4*>(v)[q] = v4;
    }
  } else {
#pragma unroll 1
    for (long long i = (long long)bid * blockDim.x + threadIdx.x; i < P; i += (long long)nblocks * blockDim.x) {
      float pi = params[i], mi = m[i], vi = v[i];
      one(i, grads[i], pi, mi, vi);
      params[i] = pi;
      m[i] = mi;
      v[i] = vi;
    }
  }
}

__global__ __launch_bounds__(256) void k_clip_adam(float* __restrict__ params,
                                                   const float* __restrict__ grads,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   long long P, const double* __restrict__ part,
                                                   float scale, float max_norm, float w1, float beta2,
                                                   float w2, float step_size, float bc2_sqrt, float eps,
                                                   float* __restrict__ stats_row, float decay = 1.0f,
                                                   float l2 = 0.0f, const double* __restrict__ lr_dev = nullptr,
                                                   double bc1 = 1.0, const int32_t* stop = nullptr) {
  clip_adam_body(params, grads, m, v, P, part, scale, max_norm, w1, beta2, w2, step_size, bc2_sqrt, eps, stats_row,
                 decay, l2, (int)blockIdx.x, (int)gridDim.x, nullptr, lr_dev, bc1, stop);
}

// Tail of optimizer step s fused with the head of step s+1: blocks [0, adam_blocks) run clip + Adam (and keep the
// padded first-layer weight copies current), the remaining blocks gather + normalise the NEXT minibatch -- it
// depends only on the rollout, the permutation and the pre-scanned normaliser trajectory, never on the parameters,
// and the activations it overwrites were last read by this step's weight-gradient launches (earlier in the stream).
// One launch and one kernel boundary less per optimizer step; same arithmetic as the two separate kernels.
struct AdamArgs {
  float* params; const float* grads; float* m; float* v; long long P; const double* part;
  float scale, max_norm, w1, beta2, w2, step_size, bc2_sqrt, eps; float* stats_row;
  const double* lr_dev; double bc1;   // adaptive schedule: the rate's device address (NULL: step_size as given) and 1 - beta1^t
  const int32_t* stop;                // KL early stopping: the stop word (NULL = off); the gather half reads GatherArgs::stop
};
__global__ __launch_bounds__(256) void k_adam_gather(const AdamArgs a, const W1Mirror mir, const GatherArgs g,
                                                     int adam_blocks) {
  // the gather blocks come first in the grid (the longer dependent chain: index -> row -> store), so that both kinds
  // are resident from the start
  const int gblocks = (int)gridDim.x - adam_blocks;
  if ((int)blockIdx.x < gblocks)
    gather_normalize_body(g, (int)blockIdx.x, gblocks);
  else
    clip_adam_body(a.params, a.grads, a.m, a.v, a.P, a.part, a.scale, a.max_norm, a.w1, a.beta2, a.w2, a.step_size,
                   a.bc2_sqrt, a.eps, a.stats_row, 1.0f, 0.0f, (int)blockIdx.x - gblocks, adam_blocks, &mir, a.lr_dev,
                   a.bc1, a.stop);
}

// KL-adaptive learning rate (rl_games AdaptiveScheduler.update, frozen_ppo.py:864-877, fed as at :624-630 with the call
// of :630 live): one wave, launched once per mini-epoch behind its last optimizer step.  kl = fp32 mean of the n_mb
// per-step KL values (stats slot 4) of the mini-epoch, as torch.mean(torch.stack(ep_kls)); the comparison and the
// rate are doubles, as in Python.  lr_state: [0] rate, [1] scratch float of the data-parallel exchange,
// [2 + 2e] / [3 + 2e] the record of mini-epoch e (KL as compared, rate after the decision).
//   mode 0: one rank -- mean and decision
//   mode 1: data parallel, before the exchange -- this rank's mean into the scratch float, no decision
//   mode 2: data parallel, after the all-reduce (SUM) of the scratch float -- kl = sum / world (fp32, :625-627), decision
// stop (KL early stopping, NULL = off): the update stopped at step *stop >= 0.  In the mini-epoch of that step the mean
// runs over its steps 0 .. *stop % nmb (the reference's ep_kls at the inner break, :630 sits between the two breaks);
// in every later one the launch is inert.
// Every store is a plain C++ store from lane 0.
__global__ __launch_bounds__(64) void k_lr_schedule(const float* __restrict__ stats_epoch, int nmb, int epoch, int mode,
                                                    int world, double kl_threshold, double lr_min, double lr_max,
                                                    double* __restrict__ lr_state, const int32_t* stop = nullptr) {
  if (threadIdx.x != 0) return;
  if (stop && stop[0] >= 0) {
    if (stop[0] / nmb != epoch) return;
    nmb = stop[0] % nmb + 1;
  }
  float* scratch = reinterpret_cast<float*>(lr_state + 1);
  float kl;
  if (mode != 2) {
    float sum = 0.f;
    for (int i = 0; i < nmb; ++i) sum += stats_epoch[(long long)i * IGI_STATS_PER_STEP + 4];
    kl = sum / (float)nmb;
    if (mode == 1) { *scratch = kl; return; }
  } else {
    kl = *scratch / (float)world;
  }
  const double k = (double)kl;
  const double cur = lr_state[0];
  double lr = cur;
  if (k > 2.0 * kl_threshold) lr = fmax(cur / 1.5, lr_min);
  if (k < 0.5 * kl_threshold) lr = fmin(cur * 1.5, lr_max);
  lr_state[0] = lr;
  lr_state[2 + 2 * epoch] = k;
  lr_state[3 + 2 * epoch] = lr;
}

// KL early stopping, data parallel: the decision from the rank-mean estimator.  The statistics block left this rank's
// fp32 mean in the scratch float, state[1]; it was all-reduced (SUM) in place; one lane divides by the world size in
// fp32 and compares as the single-rank block does -- the same bits on every rank, so every rank stops at the same step.
// A step behind a stop leaves the word alone (every rank is in that state alike).  Plain stores.
__global__ __launch_bounds__(64) void k_stop_decide(int32_t* __restrict__ state, int slot, int world, double limit) {
  if (threadIdx.x != 0) return;
  if (slot > 0 && state[0] >= 0) return;
  const float kl = reinterpret_cast<const float*>(state)[1] / (float)world;
  reinterpret_cast<float*>(state)[2 + slot] = kl;
  state[0] = ((double)kl > limit) ? slot : -1;
}

// ---------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------
static int check_state(const TeacherPlan& p, const igi_teacher_state* st) {
  if (!st || !st->params || !st->workspace) return IGI_E_BADARG;
  if (st->workspace_bytes < p.w_total) return IGI_E_WORKSPACE;
  return 0;
}
static inline bool lr_adaptive(const igi_teacher_cfg* c) { return c->lr_schedule != 0; }
static int check_lr_cfg(const igi_teacher_cfg* c, const igi_teacher_state* st) {
  if (!lr_adaptive(c)) return 0;
  if (c->lr_schedule != 1 || !(c->kl_threshold > 0.0) || !(c->lr_min > 0.0) || !(c->lr_max >= c->lr_min) || !st->lr_state ||
      !st->stats)
    return IGI_E_BADARG;
  return 0;
}

static inline bool kl_stop_on(const igi_kl_stop* ks) { return ks && ks->kl_early_stop != 0; }
// one threshold: under the adaptive schedule the stop's must be the scheduler's
static int check_ks(const igi_kl_stop* ks, const igi_teacher_state* st, const igi_teacher_cfg* c) {
  if (!kl_stop_on(ks)) return 0;
  if (ks->kl_early_stop != 1 || !(ks->kl_threshold > 0.0) || !ks->stop_state || !st->stats) return IGI_E_BADARG;
  if (c->lr_schedule != 0 && c->kl_threshold != ks->kl_threshold) return IGI_E_BADARG;
  return 0;
}
// What a data-parallel update puts between the stages of an optimizer step (teacher_update_steps).  One hook, called
// with the bucket of igi_reduce_fn's protocol, everything in the order of the update's stream:
enum ExchangeBucket {
  XB_EARLY = 0,      // behind phase 0 (two_phase only): start the all-reduce of the early ranges
  XB_LATE = 1,       // behind phase 1 / behind the whole fwd_bwd: the late ranges / the whole flat gradient
  XB_JOIN = 2,       // ahead of teacher_apply: the stream waits for what XB_EARLY and XB_LATE started
  XB_KL = 3,         // all-reduce (SUM) the mini-epoch KL, the float at st->lr_state + 1, between the scheduler's halves
  XB_ESTIMATOR = 4,  // all-reduce (SUM) the step's estimator, the float at ks->stop_state + 1, between k_sumsq_stats
};                   // and k_stop_decide
struct UpdateExchange {
  int world;         // ranks; < 1 = unknown, refused where the schedule or the stop divides by it
  float grad_scale;  // 1 / world, folded into the Adam kernel
  bool two_phase;    // fwd_bwd in two phases with XB_EARLY between them
  bool foreign;      // fn is a caller's callback: whatever it returns but 0 is IGI_E_CALLBACK; else fn returns our codes
  void* ctx;
  igi_reduce_fn fn;  // (ctx, bucket, slot)
};
static inline int exchange(const UpdateExchange* x, int bucket, int slot) {
  const int rc = x->fn(x->ctx, bucket, slot);
  return rc && x->foreign ? IGI_E_CALLBACK : rc;
}

static int teacher_prepare(const igi_teacher_cfg* c, const igi_rollout* ro,
                           const igi_teacher_state* st, int normalize_value, hipStream_t s) {
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if (!ro || !ro->rewards || !ro->values || !ro->dones || !ro->last_values || !ro->mus ||
      !ro->sigmas || !st->returns_raw || !st->advantages || !st->values_n || !st->returns_n ||
      !st->mus_w || !st->sigmas_w || (normalize_value && !st->rms_value))
    return IGI_E_BADARG;
  double* part = wsp<double>(st, p.w_prep_part);
  float* coef = wsp<float>(st, p.w_prep_coef);
  const float gamma = (float)c->gamma;
  const float gamma_tau = (float)((double)c->gamma * (double)c->tau);
  ProfScope ps(PC_PREPARE, s, 0.0, 17.0 * (double)p.Bsz + 8.0 * p.act * (double)p.Bsz * 2, /*ext=*/false);
  IGI_LAUNCH(k_gae, dim3(p.gae_blocks), dim3(PREP_THREADS), 0, s, ro->rewards, ro->values,
                     ro->dones, ro->last_values, st->returns_raw, p.N, p.T, gamma, gamma_tau, part);
  IGI_LAUNCH(k_prep_final, dim3(1), dim3(64), 0, s, part, p.gae_blocks, p.Bsz,
                     st->rms_value, c->rms_eps, coef, normalize_value);
  int nb = (int)((p.Bsz * p.act + PREP_THREADS - 1) / PREP_THREADS);
  if (nb > 2048) nb = 2048;
  IGI_LAUNCH(k_prep_norm, dim3(nb), dim3(PREP_THREADS), 0, s, ro->values, st->returns_raw,
                     ro->mus, ro->sigmas, coef, st->advantages, st->values_n, st->returns_n,
                     st->mus_w, st->sigmas_w, p.Bsz, p.act, normalize_value);
  // normaliser trajectory for the E*n_mb optimizer steps of this update (see k_rms_traj)
  if (ro->obses && ro->priv_info && st->perm && st->rms_obs && st->rms_priv) {
    const int D = p.obs + p.priv;
    double* rpart = wsp<double>(st, p.w_rms_part);
    for (int i = 0; i < p.nmb; ++i)
      IGI_LAUNCH(k_gather_stats, dim3(p.gs_blocks), dim3(GS_THREADS),
                         (size_t)p.gs_rows * (D + 2) * sizeof(float), s, ro->obses, ro->priv_info, st->perm,
                         (long long)i * p.mb, p.mb, p.N, p.T, p.obs, p.priv, p.gs_rows, wsp<float>(st, p.w_xcat),
                         p.xld, wsp<float>(st, p.w_priv), ru4(p.priv), rpart + (long long)i * p.gs_blocks * D * 2);
    IGI_LAUNCH(k_mb_moments, dim3(p.nmb), dim3(RMSF_THREADS), 0, s, rpart, p.gs_blocks, p.mb, D,
                       wsp<float>(st, p.w_moments));
    IGI_LAUNCH(k_rms_traj, dim3(1), dim3(128), 0, s, wsp<float>(st, p.w_moments), p.nmb, p.E * p.nmb,
                       p.mb, p.obs, p.priv, st->rms_obs, st->rms_priv, c->rms_eps, wsp<float>(st, p.w_traj_coef),
                       wsp<double>(st, p.w_traj_state));
  }
  return (int)hipGetLastError();
}

// W1p[net][o][c] = first trunk layer weight padded to xld columns (zeros) so the layer runs on
// the LDS-DMA kernel (k-tile 32) and its dgrad / wgrad see aligned 16-byte rows.
__global__ __launch_bounds__(256) void k_pad_w1(const float* __restrict__ params, long long o_w, long long ac_block,
                                                int u0, int u0p, int xw, int xld, float* __restrict__ w1p, int nets) {
  const int total = nets * u0p * xld;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int c = e % xld;
    const int o = (e / xld) % u0p;
    const int net = e / (xld * u0p);
    w1p[e] = (c < xw && o < u0) ? params[o_w + net * ac_block + (long long)o * xw + c] : 0.f;
  }
}

// d(latent pre-activation) = ([dZ1_actor | dZ1_critic] . W1p[:, obs:obs+LAT]) * (1 - latent^2).
// Only LAT (= 8) of the first layer's input columns need a gradient, so this is a skinny
// (mb x K) . (K x 8) product: one wave per row, each lane keeps its 16 x 8 slice of the weight in
// registers for all of its rows and the 8 row sums are wave reductions -- HBM-bound on reading dZ1
// once (a 128 x 64 MFMA tile would spend 8x the useful FLOPs on padding here).
// RAW (teacher_actor_latent_backward: the latent is the student's, there is no tanh behind it): the products themselves,
// to the dense [mb][LAT] `dxcat`; `xcat` is not read and `w1p` may be the unpadded weight (rows xld = xw floats apart).
template <int KQ, int LAT, bool RAW = false>
__global__ __launch_bounds__(256) void k_latent_dgrad(const float* __restrict__ dz, int ldz,
                                                      const float* __restrict__ w1p, int xld, int obs,
                                                      const float* __restrict__ xcat, float* __restrict__ dxcat,
                                                      int mb, int rows_per_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float w[KQ][4][LAT];
#pragma unroll
  for (int q = 0; q < KQ; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 4 * lane + 256 * q + i;
#pragma unroll
      for (int j = 0; j < LAT; ++j) w[q][i][j] = w1p[(long long)k * xld + obs + j];
    }
  const int gw = blockIdx.x * 4 + wave;
  for (int it = 0; it < rows_per_wave; it += 4) {  // four rows in flight: their loads are independent
    const int row0 = gw * rows_per_wave + it;
    if (row0 >= mb) break;
    float4 v[4][KQ];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(row0 + r, mb - 1);
#pragma unroll
      for (int q = 0; q < KQ; ++q)
        v[r][q] = *reinterpret_cast<const float4*>(dz + (long long)row * ldz + 4 * lane + 256 * q);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + r;
      float acc[LAT];
#pragma unroll
      for (int j = 0; j < LAT; ++j) acc[j] = 0.f;
#pragma unroll
      for (int q = 0; q < KQ; ++q)
#pragma unroll
        for (int j = 0; j < LAT; ++j)
          acc[j] += ((v[r][q].x * w[q][0][j] + v[r][q].y * w[q][1][j]) + v[r][q].z * w[q][2][j]) + v[r][q].w * w[q][3][j];
#pragma unroll
      for (int j = 0; j < LAT; ++j) acc[j] = wave_sum(acc[j]);
      if (row < mb && it + r < rows_per_wave) {
#pragma unroll
        for (int j = 0; j < LAT; ++j) {
          if (lane == j) {
            if constexpr (RAW) {
              dxcat[(long long)row * LAT + j] = acc[j];
            } else {
              const float t = xcat[(long long)row * xld + obs + j];
              dxcat[(long long)row * xld + obs + j] = acc[j] * (1.0f - t * t);
            }
          }
        }
      }
    }
  }
}

// Fused tail of the backward pass around the 8-wide latent: the latent data gradient, plus the last
// env_mlp layer's data gradient (d pre-activation of the previous env layer, times tanh') and its
// weight / bias gradient.  All are rank-8 products over rows the block already holds, so they ride in
// one HBM-bound kernel instead of an MFMA launch padded 8x plus two latency-bound generic GEMMs.
//   dze3[j]     = (sum_k dZ1[row][k] * W1p[k][obs+j]) * (1 - latent_j^2)
//   dze2[row][c]= (sum_j dze3[j] * We3[j][c]) * (1 - e2[row][c]^2)
//   dWe3[j][c] += dze3[j] * e2[row][c] ;  dbe3[j] += dze3[j]      (per-block partials, reduced later)
// A block takes 32 rows.  Phase 1 is a matrix-pipe product: the dZ1 rows stream through LDS in 256-column chunks
// (coalesced 16-byte loads, next chunk prefetched into registers), the eight weight rows sit in LDS transposed,
// and each wave multiplies 16 rows by the eight outputs with v_mfma_f32_16x16x4_f32 (see the loop).  Measured: the
// chunk loop runs at the stream's rate (67 MB in ~14 us); the other ~13 us of the kernel are launch, the weight
// copy, phase 2 and the block reduction.  Phase 2 gives each wave its 8 rows for the rank-8 updates; its operands
// are requested before phase 1.
constexpr int LATB_ROWS = 32;
constexpr int LATB_CH = 256;            // columns per staged chunk
constexpr int LATB_LD = LATB_CH + 4;    // padded row stride (floats): rows land on distinct LDS banks
// PARTS: phase 1 already happened inside the data-gradient tiles that produced dZ1 (GemmArgs::rowdot_*): `dz` then
// points at their per-tile row dots [ldz tiles][mb][8], which are added in tile order; dZ1 is not read again.
template <int MAXJ, bool PARTS = false>
__global__ __launch_bounds__(256) void k_latent_bwd(const float* __restrict__ dz, int ldz, int K2,
                                                    const float* __restrict__ wlat, int xld, int obs,
                                                    const float* __restrict__ xcat, float* __restrict__ dxcat,
                                                    const float* __restrict__ e2, int lde, int H2,
                                                    const float* __restrict__ We3, float* __restrict__ dze2,
                                                    float* __restrict__ partial, int mb) {
  constexpr int LAT = 8;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int K2p = (K2 + LATB_CH - 1) / LATB_CH * LATB_CH;
  const int wld = K2p + 4;
  float* wt = sm;                               // [LAT][wld]: latent columns of W1p, transposed, zero beyond K2
  float* tile = wt + LAT * wld;                 // [LATB_ROWS][LATB_LD]; reused for the final block reduction
  float* psum = tile + LATB_ROWS * LATB_LD;     // [LATB_ROWS][LAT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (!PARTS)
  for (int e = tid; e < LAT * K2p / 4; e += 256) {  // wlat is [LAT][K2p], already zero beyond K2: coalesced copy
    const int j = e / (K2p / 4), k4 = e - j * (K2p / 4);
    *reinterpret_cast<float4*>(wt + j * wld + 4 * k4) = *reinterpret_cast<const float4*>(wlat + (long long)j * K2p + 4 * k4);
  }
  float we[LAT][MAXJ], gw[LAT][MAXJ];
#pragma unroll
  for (int j = 0; j < LAT; ++j)
#pragma unroll
    for (int jj = 0; jj < MAXJ; ++jj) {
      const int c = lane + 64 * jj;
      we[j][jj] = (c < H2) ? We3[j * H2 + c] : 0.f;
      gw[j][jj] = 0.f;
    }
  float gb = 0.f;  // lane j (< 8) accumulates dbe3[j]
  auto rl = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
  const int row0 = blockIdx.x * LATB_ROWS;
  // phase 1 on the matrix pipe: per staged 256-column chunk, wave w multiplies rows 16 (w & 1) .. +15 by the eight
  // weight rows over every second 16-k slice (starting at w >> 1) with v_mfma_f32_16x16x4_f32: lane (m = lane & 15,
  // q = lane >> 4) supplies A[m][4q + t] and B[4q + t][n = m] to the t-th instruction of a slice, i.e. one 16-byte
  // LDS read of the staged dZ1 row m and one of weight row n per four MFMAs (the VALU version needed two 16-byte
  // reads per four FMAs per thread).  Outputs n >= 8 multiply zeros.  The two k-halves meet in LDS afterwards.
  // phase-2 operands of this wave's eight rows are requested now: their latency hides under phase 1
  float tl8[8], ee8[8][MAXJ];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int row = min(row0 + wave * 8 + r, mb - 1);
    tl8[r] = xcat[(long long)row * xld + obs + (lane & 7)];
#pragma unroll
    for (int jj = 0; jj < MAXJ; ++jj) {
      const int c = lane + 64 * jj;
      ee8[r][jj] = (c < H2) ? e2[(long long)row * lde + c] : 0.f;
    }
  }
  if constexpr (!PARTS) {
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  const int fm = lane & 15, fq = lane >> 4, rh = wave & 1, kh = wave >> 1;
  const bool bvalid = fm < LAT;
  f32x4_t facc = {0.f, 0.f, 0.f, 0.f};
  float4 ld[8];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      const int r = idx >> 6, c4 = idx & 63;
      const int row = min(row0 + r, mb - 1);
      const int k = c0 + 4 * c4;
      ld[i] = (k < K2) ? *reinterpret_cast<const float4*>(dz + (long long)row * ldz + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  fetch(0);
  for (int c0 = 0; c0 < K2p; c0 += LATB_CH) {
    __syncthreads();  // previous chunk consumed (and wt written, first time round)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<float4*>(tile + (idx >> 6) * LATB_LD + 4 * (idx & 63)) = ld[i];
    }
    __syncthreads();
    if (c0 + LATB_CH < K2p) fetch(c0 + LATB_CH);  // in flight during the arithmetic below
    const float* xr = tile + (rh * 16 + fm) * LATB_LD + 4 * fq;
    const float* wr = wt + min(fm, LAT - 1) * wld + c0 + 4 * fq;
#pragma unroll
    for (int c = 0; c < LATB_CH / 32; ++c) {       // this wave's 16-k slices: kh, kh + 2, ...
      const int off = 16 * (kh + 2 * c);
      const float4 x = *reinterpret_cast<const float4*>(xr + off);
      float4 wv = *reinterpret_cast<const float4*>(wr + off);
      if (!bvalid) wv = make_float4(0.f, 0.f, 0.f, 0.f);
      facc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, wv.x, facc, 0, 0, 0);
      facc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, wv.y, facc, 0, 0, 0);
      facc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, wv.z, facc, 0, 0, 0);
      facc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, wv.w, facc, 0, 0, 0);
    }
  }
  // C/D layout: register r of lane (m, q) is D[row 4q + r][output m]; k-half 1 parks its part in LDS, half 0 adds
  __syncthreads();                                 // the staging tile is free
  float* khalf = tile;                             // [LATB_ROWS][LAT]
  if (kh == 1 && bvalid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) khalf[(rh * 16 + 4 * fq + r) * LAT + fm] = facc[r];
  }
  __syncthreads();
  if (kh == 0 && bvalid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = (rh * 16 + 4 * fq + r) * LAT + fm;
      psum[e] = facc[r] + khalf[e];
    }
  }
  __syncthreads();
  } else {
    // thread (row = tid / 8, j = tid % 8) adds the tiles' row dots in tile order
    const int r_ = tid >> 3, j_ = tid & 7;
    const int row_ = min(row0 + r_, mb - 1);
    float acc_ = 0.f;
    for (int t0 = 0; t0 < ldz; t0 += 8) {   // eight tiles' partials per round trip (one each was the kernel's duration)
      float v_[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v_[u] = dz[((long long)min(t0 + u, ldz - 1) * mb + row_) * LAT + j_];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < ldz) acc_ += v_[u];
    }
    psum[r_ * LAT + j_] = acc_;
    __syncthreads();
  }
  // ---- phase 2: wave handles rows wave*8 .. wave*8+7
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int rr = wave * 8 + r;
    const int row = row0 + rr;
    const bool live = row < mb;
    const float ps = psum[rr * LAT + (lane & 7)];
    const float dl = (live && lane < LAT) ? ps * (1.0f - tl8[r] * tl8[r]) : 0.f;  // lane j: dze3[j]
    if (live && lane < LAT) {
      dxcat[(long long)row * xld + obs + lane] = dl;
      gb += dl;
    }
    float d[LAT];
#pragma unroll
    for (int j = 0; j < LAT; ++j) d[j] = rl(dl, j);
#pragma unroll
    for (int jj = 0; jj < MAXJ; ++jj) {
      const int c = lane + 64 * jj;
      float sacc = 0.f;
#pragma unroll
      for (int j = 0; j < LAT; ++j) {
        sacc = fmaf(d[j], we[j][jj], sacc);
        gw[j][jj] = fmaf(d[j], ee8[r][jj], gw[j][jj]);
      }
      if (live && c < H2) dze2[(long long)row * lde + c] = sacc * (1.0f - ee8[r][jj] * ee8[r][jj]);
    }
  }
  // block partial [LAT*H2 | LAT] (the staging tile is free now)
  __syncthreads();
  float* red = tile;
  const int pc = LAT * H2 + LAT;
  float* mine_p = red + wave * pc;
#pragma unroll
  for (int j = 0; j < LAT; ++j)
#pragma unroll
    for (int jj = 0; jj < MAXJ; ++jj) {
      const int c = lane + 64 * jj;
      if (c < H2) mine_p[j * H2 + c] = gw[j][jj];
    }
  if (lane < LAT) mine_p[LAT * H2 + lane] = gb;
  __syncthreads();
  for (int e = threadIdx.x; e < pc; e += blockDim.x)
    partial[(long long)blockIdx.x * pc + e] = (red[e] + red[pc + e]) + (red[2 * pc + e] + red[3 * pc + e]);
}

// forward through env_mlp -> xcat -> actor/critic trunk for `rows` rows already staged
// (normalised) in priv_g / xcat.
// (the contact-encoder arguments of this call, filled by contact_args: required in contact mode)
static int trunk_forward(const TeacherPlan& p, const igi_teacher_state* st, int rows, bool pad_w1, hipStream_t s,
                         int nl_run = -1,   // nl_run: trunk layers to run (the training step leaves the last one to k_trunk_loss)
                         const ContactArgs* ct = nullptr) {
  if (nl_run < 0) nl_run = p.nl;
  if (p.ct_P > 0 && !ct) return IGI_E_BADARG;
  const float* P = st->params;
  float* priv_g = wsp<float>(st, p.w_priv);
  float* xcat = wsp<float>(st, p.w_xcat);
  float* w1p = wsp<float>(st, p.w_w1p);
  const long long mbs = p.mb;
  if (pad_w1) {
    ProfScope ps(PC_OTHER, s, 0.0, 8.0 * p.nets * p.u0p * p.xld);
    IGI_LAUNCH(k_pad_w1, dim3((p.nets * p.u0p * p.xld + 255) / 256), dim3(256), 0, s, P, p.o_acW[0],
                       p.ac_block, p.u[0], p.u0p, p.xw, p.xld, w1p, p.nets);
  }
  // env_mlp: tanh after every layer, the last one lands in xcat[:, obs:]
  const float* in = priv_g;
  int ldin = ru4(p.priv);
  bool env_done = p.ct_only != 0;   // only_contact: the privileged embedding is not used (models_split.py:176-177)
  int first_trunk_layer = 0;
  // round 6: env_mlp AND the first trunk layer of both nets as one persistent launch (fwd12.h); other shapes keep
  // k_env_fwd (or the per-layer launches) + the layer's own launch below
  // (k_fwd12 runs the first trunk layer of TWO nets: a shared trunk declines it and takes the launches below)
  if (env_fused() && p.nets == 2 && p.npl == 3 && p.ct_P == 0 && nl_run >= 1 && rows >= 2048 && !bf16_mode() &&
      fwd12_supported(p.priv, p.pu[0], p.pu[1], p.pu[2], p.obs, p.xld, p.u[0]) && p.u0p == p.u[0]) {
    Fwd12Args f;
    f.priv = priv_g; f.ldp = ldin; f.xcat = xcat; f.ldx = p.xld; f.M = rows; f.obs = p.obs;
    f.eW1 = P + p.o_envW[0]; f.eb1 = P + p.o_envB[0]; f.eW2 = P + p.o_envW[1]; f.eb2 = P + p.o_envB[1];
    f.eW3 = P + p.o_envW[2]; f.eb3 = P + p.o_envB[2];
    f.w1p = w1p; f.tb1 = P + p.o_acB[0]; f.ac_block = p.ac_block;
    f.e1 = wsp<float>(st, p.w_e[0]); f.lde1 = ru4(p.pu[0]);
    f.e2 = wsp<float>(st, p.w_e[1]); f.lde2 = ru4(p.pu[1]);
    f.h1 = wsp<float>(st, p.w_h[0]); f.ldh = ru4(p.u[0]); f.sH = mbs * ru4(p.u[0]);
    if (fwd12_forward(f, s) == hipSuccess) { env_done = true; first_trunk_layer = 1; }
  }
  // (the fused kernel is one workgroup per 64 rows with a fixed ~20 us chain: at the rollout's 4096 rows it fills a
  // quarter of the chip and the per-layer launches win -- measured 8.4 -> 8.0 ms per 32-step rollout)
  if (!env_done && env_fused() && p.npl == 3 && rows >= 8192 && !bf16_mode()) {
    // the whole env_mlp of a 64-row block in one workgroup (env_mlp.h); other shapes run layer by layer below
    // (an fp32 kernel: in the bf16-input mode the layers go through gemm() like every other fused class's, so the
    // forward of a layer and its backward products are under the switch together)
    EnvFwdArgs a;
    a.priv = priv_g; a.ldp = ldin;
    a.W1 = P + p.o_envW[0]; a.b1 = P + p.o_envB[0];
    a.W2 = P + p.o_envW[1]; a.b2 = P + p.o_envB[1];
    a.W3 = P + p.o_envW[2]; a.b3 = P + p.o_envB[2];
    a.e1 = wsp<float>(st, p.w_e[0]); a.lde1 = ru4(p.pu[0]);
    a.e2 = wsp<float>(st, p.w_e[1]); a.lde2 = ru4(p.pu[1]);
    a.out = xcat + p.obs; a.ldo = p.xld;
    a.M = rows; a.K1 = p.priv; a.N1 = p.pu[0]; a.N2 = p.pu[1]; a.N3 = p.pu[2]; a.ldw2 = p.pu[0];
    env_done = env_mlp_forward(a, s) == hipSuccess;
  }
  for (int l = 0; l < p.npl && !env_done; ++l) {
    GemmArgs g;
    g.A = in; g.lda = ldin;
    g.B = P + p.o_envW[l]; g.ldb = env_in(p, l);
    g.bias = P + p.o_envB[l];
    g.M = rows; g.N = p.pu[l]; g.K = env_in(p, l);
    if (l == p.npl - 1) { g.C = xcat + p.obs; g.ldc = p.xld; }
    else { g.C = wsp<float>(st, p.w_e[l]); g.ldc = ru4(p.pu[l]); }
    g.epilogue = EPI_BIAS_TANH;
    if (l == p.npl - 2 && p.pu[l + 1] <= 8) {
      // the <= 8-wide latent layer rides in this layer's epilogue (one launch less per step)
      GemmArgs gh = g;
      gh.head_W = P + p.o_envW[l + 1]; gh.head_b = P + p.o_envB[l + 1];
      gh.head_out = xcat + p.obs; gh.head_ld = p.xld; gh.head_n = p.pu[l + 1];
      if (gemm_with_head(gh, s) == hipSuccess) break;
    }
    IGI_HIP_TRY(gemm(g, true, true, s));
    in = g.C; ldin = g.ldc;
  }
  if (p.ct_P > 0) {   // contact embedding -> xcat[:, ct_col:ct_col + ct_E]
    const hipError_t e = contact_forward(*ct, s);
    if (e != hipSuccess) return (int)e;
  }
  // actor + critic, batched (critic parameters sit ac_block floats after the actor's)
  in = xcat; ldin = p.xld;
  long long sIn = 0;
  if (first_trunk_layer == 1) { in = wsp<float>(st, p.w_h[0]); ldin = ru4(p.u[0]); sIn = mbs * ru4(p.u[0]); }
  for (int l = first_trunk_layer; l < nl_run; ++l) {
    GemmArgs g;
    g.A = in; g.lda = ldin; g.sA = sIn;
    if (l == 0) { g.B = w1p; g.ldb = p.xld; g.sB = (long long)p.u0p * p.xld; g.K = p.xld; g.flop_credit = (double)p.xw / p.xld; }
    else { g.B = P + p.o_acW[l]; g.ldb = ac_in(p, l); g.sB = p.ac_block; g.K = ac_in(p, l); }
    g.bias = P + p.o_acB[l]; g.sBias = p.ac_block;
    g.M = rows; g.N = p.u[l];
    g.C = wsp<float>(st, p.w_h[l]); g.ldc = ru4(p.u[l]); g.sC = mbs * ru4(p.u[l]);
    g.nbatch = p.nets;
    g.epilogue = EPI_BIAS_TANH;
    IGI_HIP_TRY(gemm(g, true, true, s));
    in = g.C; ldin = g.ldc; sIn = g.sC;
  }
  return 0;
}

// phase -1: the whole step.  Data-parallel runs split it so that the gradient all-reduce of the big
// bucket overlaps the rest of backward (frozen_ppo.py:586-603 reduces everything after backward).  The cut follows the
// backward levels, so both phases launch exactly the kernels of the unsplit step (the only extra launch is the second
// call of k_slab_reduce):
//   phase 0: gather, forward, loss, trunk backward down to dZ of the FIRST trunk layer, sum of the split-K slabs of the
//            heads and of trunk layers >= 1       -> the EARLY bucket is final: actor layers >= 1 | critic layers >= 1,
//            value, mu  (two ranges of the flat gradient: the critic's first layer lies between them)
//   phase 1: latent + env_mlp backward with the first trunk layer's weight gradient riding in the env level's grid,
//            sum of the remaining slabs          -> the LATE bucket: sigma, env_mlp, actor layer 0 | critic layer 0
struct GradBuckets { long long off[4], len[4]; };   // [0], [1]: early; [2], [3]: late (a length may be 0)
static GradBuckets grad_buckets(const TeacherPlan& p) {
  const long long a0 = p.o_acW[0], blk = p.ac_block;
  const long long rel1 = p.nl > 1 ? p.o_acW[1] - p.o_acW[0] : blk;   // first trunk layer's share of a net's block
  GradBuckets b;
  b.off[0] = a0 + rel1;        b.len[0] = blk - rel1;                 // actor layers >= 1
  b.off[1] = a0 + blk + rel1;  b.len[1] = p.P - b.off[1];             // critic layers >= 1, value, mu
  b.off[2] = 0;                b.len[2] = a0 + rel1;                  // sigma, env_mlp, actor layer 0
  b.off[3] = a0 + blk;         b.len[3] = rel1;                       // critic layer 0
  if (p.nets == 1) {   // no critic block: the early bucket is ONE range, both critic ranges are empty
    b.len[0] = p.P - b.off[0];                                        // actor layers >= 1, value, mu
    b.off[1] = p.P; b.len[1] = 0;
    b.len[3] = 0;
  }
  return b;
}

static GatherArgs gather_args(const TeacherPlan& p, const igi_rollout* ro, const igi_teacher_state* st, int mb_index,
                              int step_slot) {
  const int D = p.obs + p.priv;
  GatherArgs a;
  a.obses = ro->obses; a.priv_info = ro->priv_info; a.perm = st->perm;
  a.start = (long long)mb_index * p.mb; a.mb = p.mb; a.N = p.N; a.T = p.T; a.obs = p.obs; a.priv = p.priv;
  a.rows_per_block = p.gs_rows; a.gather_blocks = p.gs_blocks;
  a.coef = wsp<float>(st, p.w_traj_coef) + (long long)step_slot * 2 * D;
  a.state_row = wsp<double>(st, p.w_traj_state) + (long long)step_slot * (2 * D + 2);
  a.rms_obs = st->rms_obs; a.rms_priv = st->rms_priv;
  a.xcat = wsp<float>(st, p.w_xcat); a.xld = p.xld; a.xw = p.xw;
  a.priv_g = wsp<float>(st, p.w_priv); a.pld = ru4(p.priv);
  a.params = st->params; a.o_w = p.o_acW[0]; a.ac_block = p.ac_block; a.u0 = p.u[0]; a.u0p = p.u0p;
  a.w1p = wsp<float>(st, p.w_w1p);
  a.wlat = p.lat_fused ? wsp<float>(st, p.w_wlat) : (float*)nullptr;
  a.K2p = (p.nets * p.u0p + 255) / 256 * 256;
  a.nets = p.nets;
  return a;
}

// Data gradient of trunk layer l (> 0) into layer l-1: dZ_{l-1} = (dZ_l . W_l) * tanh'(h_{l-1}), both nets batched.
// with_rowdot (l == 1): the dZ1 tiles also emit their share of dZ1 . W1[:, latent columns] (GemmArgs::rowdot_*).
static GemmArgs trunk_dgrad_args(const TeacherPlan& p, const igi_teacher_state* st, int l, bool with_rowdot) {
  const long long mbs = p.mb;
  GemmArgs g;
  g.A = wsp<float>(st, p.w_dh[l]); g.lda = dz_ld(p, l); g.sA = dz_stride(p, l);
  g.B = st->params + p.o_acW[l]; g.ldb = ac_in(p, l); g.sB = p.ac_block;
  g.M = p.mb; g.N = ac_in(p, l); g.K = p.u[l];
  g.C = wsp<float>(st, p.w_dh[l - 1]); g.ldc = dz_ld(p, l - 1); g.sC = dz_stride(p, l - 1);
  g.aux = wsp<float>(st, p.w_h[l - 1]); g.ldaux = ru4(p.u[l - 1]); g.sAux = mbs * ru4(p.u[l - 1]);
  g.nbatch = p.nets;
  g.epilogue = EPI_TANHGRAD;
  if (with_rowdot) {
    g.rowdot_W = wsp<float>(st, p.w_wlat); g.rowdot_ld = (2 * p.u0p + 255) / 256 * 256; g.rowdot_kz = p.u0p;
    g.rowdot_out = wsp<float>(st, p.w_lat_rowdot);
    if (p.lw_parts > 0 && l == 1) {
      float* slab = wsp<float>(st, p.w_slab);
      const int out0 = p.u[0];
      g.lw_X = wsp<float>(st, p.w_xcat); g.lw_ldx = p.xld; g.lw_xw = p.xw; g.lw_chain = p.lw_chain;
      g.lw_out = slab + p.s_acW[0]; g.lw_sPart = 2LL * out0 * p.xld; g.lw_sNet = (long long)out0 * p.xld;
      g.lw_bias = slab + p.s_acB[0]; g.lw_bsPart = 2LL * out0; g.lw_bsNet = out0;
    }
  }
  return g;
}

// What one step launches where the plan alone does not say: resolved ONCE per call of teacher_fwd_bwd, every stage reads it.
// The backward through the last env layer into the latent, in order of precedence: inside the env level's row-block kernel
// (rowblock.h, LATZ: no launch of its own) | k_latent_bwd<., true> from the row dots the dZ1 tiles emitted | k_latent_bwd<., false>
// over dZ1 itself | k_latent_dgrad<KQ, 8> | the EPI_TANHGRAD product over all xld columns
enum LatentPath { LAT_ENV_LEVEL, LAT_BWD_PARTS, LAT_BWD_DZ1, LAT_DGRAD, LAT_GENERIC };
struct StepPaths {
  bool rowdot, latz, lw;   // the dZ1 tiles emit the latent row dots; the plan's latz / lw_parts, live only with them
  LatentPath latent;
  // profiler class (PC_WGRAD_MULTI + .) of the level launch of trunk / env layer l and of the closing weight-gradient group
  int cls_trunk[IGI_MAX_LAYERS], cls_env[IGI_MAX_LAYERS], cls_closing;
};
static StepPaths resolve_paths(const TeacherPlan& p, const igi_teacher_state* st) {
  StepPaths q;
  // The latent gradient's K = 2*u0 contraction can ride in the tiles of the data gradient that produces dZ1 (no second
  // pass over its 67 MB): needs the level-fused multi kernel for that product.  Decided from the plan and the state's
  // addresses alone, with the very predicate the launcher applies (gemm_multi_dgrad_ok), so that both halves of a phased
  // step agree and the launch can never decline row dots the plan counted on (it falls back to k_latent_bwd<., false>).
  // (two nets only: the tiles' row dots and k_latent_bwd<., true> index the partials [tile][net]; a shared trunk's dZ1 goes
  // through k_latent_bwd<., false>, which is generic in K2 = nets * u0p)
  q.rowdot = false;
  if (p.nets == 2 && p.lat_fused && p.nl >= 2 && !bf16_mode() && p.mb >= 4) {
    GemmArgs g = trunk_dgrad_args(p, st, 1, true);
    q.rowdot = gemm_multi_dgrad_ok(g);
  }
  q.latz = p.latz && q.rowdot;
  q.lw = p.lw_parts > 0 && q.rowdot;
  const int K2 = p.nets * p.u0p;
  q.latent = p.lat_fused ? (q.latz ? LAT_ENV_LEVEL : q.rowdot ? LAT_BWD_PARTS : LAT_BWD_DZ1)
                         : (p.latent == 8 && p.ct_P == 0 && K2 % 256 == 0 && K2 <= 1024) ? LAT_DGRAD : LAT_GENERIC;
  for (int l = 0; l < IGI_MAX_LAYERS; ++l) {
    q.cls_trunk[l] = (p.nl == 3) ? (l == 2 ? 0 : 1) : 4;
    q.cls_env[l] = (p.npl == 3 && l == 1) ? 2 : 4;
  }
  q.cls_closing = (p.npl == 3) ? ((p.rb_env[1] && !q.lw) ? 5 : 3) : 4;   // (launched by the phase that runs the env stage)
  return q;
}
// the weight-gradient products that wait for the next level launch: they cross the trunk, latent and env stages
struct PendingWgrads { GemmArgs g[2 * IGI_MAX_LAYERS]; int n = 0; };

// the contact encoder of a minibatch (perm != nullptr: rows start.. of the permutation over the (T, N, P) arena) or of
// `rows` plain rows (perm == nullptr, T = 1)
static ContactArgs contact_args(const TeacherPlan& p, const igi_teacher_state* st, const float* contacts,
                                const int64_t* perm, long long start, int rows) {
  ContactArgs a;
  const float* P = st->params;
  a.C = contacts; a.perm = perm; a.start = start; a.rows = rows;
  a.N = perm ? p.N : rows; a.T = perm ? p.T : 1; a.P = p.ct_P; a.E = p.ct_E;
  a.W1 = P + p.o_ctW1; a.b1 = P + p.o_ctB1; a.W2 = P + p.o_ctW2; a.b2 = P + p.o_ctB2;
  a.H = wsp<float>(st, p.w_ct_h);
  a.out = wsp<float>(st, p.w_xcat) + p.ct_col; a.ldo = p.xld;
  a.dZ = wsp<float>(st, p.w_dxcat) + p.ct_col; a.ldz = p.xld;
  a.part = wsp<float>(st, p.w_ct_part); a.rec = p.ct_rec;
  return a;
}

// ---- the stages of one step (teacher_fwd_bwd below), each on (plan, paths, state, ...) -------------------------------
// gather + normalise with this step's pre-scanned running statistics (experience.py:207-226; frozen_ppo.py:521-522)
// + publish the running state + refresh the padded first-layer weight
static void gather_stage(const TeacherPlan& p, const igi_rollout* ro, const igi_teacher_state* st, int mb_index, int step_slot,
                         const int32_t* stop, hipStream_t s) {
  ProfScope ps(PC_GATHER_NORMALIZE, s, 0.0, 8.0 * (double)p.mb * (p.obs + p.priv) + 8.0 * p.mb);
  const int pad_blocks = 16;
  GatherArgs ga = gather_args(p, ro, st, mb_index, step_slot);
  ga.stop = stop;
  IGI_LAUNCH(k_gather_normalize, dim3(p.gs_blocks + pad_blocks), dim3(GS_THREADS), 0, s, ga);
}

// backward through the actor / critic trunk.  Level fusion: the weight gradient of layer l and the data
// gradient INTO layer l-1 both consume dZ_l and are independent of each other, so they share one grid
// (gemm_level -> gemm_dma_wgrad_multi_kernel: the data-gradient tiles lead, the weight-gradient workgroups fill
// their fill / drain bubbles).  The first trunk layer's weight gradient rides with the env_mlp data gradient: it is left
// pending here (phase 1; the levels above it are phase 0).
static int trunk_backward(const TeacherPlan& p, const StepPaths& q, const igi_teacher_state* st, bool do0, bool do1,
                          PendingWgrads& pend, hipStream_t s) {
  const float* P = st->params;
  const int mb = p.mb;
  float* slab = wsp<float>(st, p.w_slab);
  for (int l = p.nl - 1; l >= 0; --l) {
    if (l > 0 && !do0) continue;
    const bool do_wgrad = l > 0 ? do0 : do1;   // the first layer's weight gradient belongs to phase 1 (env level's grid)
    const int out = p.u[l];
    const int in = (l == 0) ? p.xld : ac_in(p, l);  // layer 0 sees the zero-padded xcat
    const float* dz = wsp<float>(st, p.w_dh[l]);
    const int ldz = dz_ld(p, l);
    const long long sZ = dz_stride(p, l);
    const float* x = (l == 0) ? wsp<float>(st, p.w_xcat) : wsp<float>(st, p.w_h[l - 1]);
    const int ldx = (l == 0) ? p.xld : ru4(p.u[l - 1]);
    const long long sX = (l == 0) ? 0 : (long long)mb * ldx;
    if (p.rb_ac[l]) {
      // this level as one persistent row-block kernel: dZ_l and h_{l-1} cross the chip once, the weight gradient leaves
      // as rb_ac[l] partials per net (rowblock.h)
      RbLevelArgs r;
      r.dZ = dz; r.ldz = ldz; r.sZ = sZ;
      r.W = P + p.o_acW[l]; r.ldw = in; r.sW = p.ac_block;
      r.X = x; r.ldx = ldx; r.sX = sX;
      r.dX = wsp<float>(st, p.w_dh[l - 1]); r.lddx = dz_ld(p, l - 1); r.sdX = dz_stride(p, l - 1);
      r.dWp = slab + p.s_acW[l]; r.ldwp = in; r.sWpart = (long long)p.nets * out * in; r.sWnet = (long long)out * in;
      r.dBp = slab + p.s_acB[l]; r.sBpart = (long long)p.nets * out; r.sBnet = out;
      r.rows = mb; r.IN = in; r.nets = p.nets; r.ranges = p.rb_ac[l];
      const hipError_t e = rb_level_backward(r, s, PC_RB_TRUNK);
      if (e == hipErrorNotSupported) return IGI_E_UNSUPPORTED;   // (alignment: the plan cannot see the caller's pointers)
      IGI_HIP_TRY(e);
      continue;
    }
    if (do_wgrad && !(l == 0 && q.lw)) {  // wgrad: dW[out][in] = dZ^T X, bias = column sums of dZ
      GemmArgs g;
      g.A = dz; g.lda = ldz; g.sA = sZ;
      g.B = x; g.ldb = ldx; g.sB = sX;
      g.M = out; g.N = in; g.K = mb;
      g.C = slab + p.s_acW[l]; g.ldc = in; g.sC = (long long)out * in;
      g.Cbias = slab + p.s_acB[l]; g.sCbias = out;
      g.nbatch = p.nets; g.splitk = p.sk_ac[l];
      if (l == 0) g.flop_credit = (double)p.xw / p.xld;   // the zero-padded input columns carry no algorithmic work
      g.sCsplit = (long long)p.nets * out * in; g.sCbiasSplit = (long long)p.nets * out;
      pend.g[pend.n++] = g;
    }
    if (l > 0) {  // dgrad into the previous hidden layer, times tanh'
      // (l == 1 with row dots: the dZ1 tiles also emit their share of dZ1 . W1[:, latent columns])
      const GemmArgs g = trunk_dgrad_args(p, st, l, l == 1 && q.rowdot);
      // this layer's weight gradient needs the same dZ: it shares the data gradient's launch (gemm_level)
      IGI_HIP_TRY(gemm_level(g, pend.g, pend.n, s, q.cls_trunk[l]));
      pend.n = 0;
    }
  }
  return 0;
}

// k_latent_bwd<MAXJ, PARTS> from src = dZ1 (src_ld its leading dimension) or, PARTS, the dZ1 tiles' row-dot partials
// (src_ld = their number); the LDS limit of an instantiation is raised once
template <int MAXJ, bool PARTS>
static int launch_latent_bwd(const TeacherPlan& p, const igi_teacher_state* st, const float* src, int src_ld, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    IGI_HIP_TRY(hipFuncSetAttribute((const void*)k_latent_bwd<MAXJ, PARTS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  const int H2 = p.pu[p.npl - 2], K2 = p.nets * p.u0p, K2p = (K2 + LATB_CH - 1) / LATB_CH * LATB_CH;
  size_t tile_f = (size_t)LATB_ROWS * LATB_LD;
  if (tile_f < (size_t)4 * (8 * H2 + 8)) tile_f = (size_t)4 * (8 * H2 + 8);
  const size_t shm = sizeof(float) * (8 * (size_t)(K2p + 4) + tile_f + LATB_ROWS * 8);
  IGI_LAUNCH((k_latent_bwd<MAXJ, PARTS>), dim3(p.lat_blocks), dim3(256), shm, s, src, src_ld, K2, wsp<float>(st, p.w_wlat), p.xld,
             p.obs, wsp<float>(st, p.w_xcat), wsp<float>(st, p.w_dxcat), wsp<float>(st, p.w_e[p.npl - 2]), ru4(H2), H2,
             st->params + p.o_envW[p.npl - 1], wsp<float>(st, p.w_de[p.npl - 2]), wsp<float>(st, p.w_lat_part), p.mb);
  return 0;
}

// d(xcat) = [dZ1_actor | dZ1_critic] . [W1a ; W1c] (one contraction, K = 2*u0p), times tanh' of xcat: columns
// obs..obs+latent-1 are d(pre-activation) of the last env_mlp layer; the other columns (observations, padding) are never
// read.  Then the contact encoder's backward from its columns.
static int latent_backward(const TeacherPlan& p, const StepPaths& q, const igi_teacher_state* st, const ContactArgs& cta,
                           hipStream_t s) {
  const int mb = p.mb, K2 = p.nets * p.u0p, ldz = dz_ld(p, 0);
  const long long mbs = mb;
  const float* dz = wsp<float>(st, p.w_dh[0]);
  float *xcat = wsp<float>(st, p.w_xcat), *dxcat = wsp<float>(st, p.w_dxcat), *w1p = wsp<float>(st, p.w_w1p);
  switch (q.latent) {
    case LAT_ENV_LEVEL:   // (LATZ: the env level's row-block kernel forms dZ of the second env layer from the row dots itself)
      break;
    case LAT_BWD_PARTS:
    case LAT_BWD_DZ1: {
      const int H2 = p.pu[p.npl - 2], tiles = p.lat_tiles;
      const bool parts_path = q.latent == LAT_BWD_PARTS;   // the K2-wide contraction then happened in the dZ1 tiles
      ProfScope ps(PC_LATENT_BWD, s, (parts_path ? 0.0 : 2.0 * mbs * K2 * 8) + 6.0 * mbs * 8 * H2,
                   4.0 * mbs * ((parts_path ? 8.0 * tiles : (double)K2) + 3 * H2));
      const bool j2 = (H2 + 63) / 64 <= 2;
      const float* parts = wsp<float>(st, p.w_lat_rowdot);
      int rc;
      if (parts_path) rc = j2 ? launch_latent_bwd<2, true>(p, st, parts, tiles, s) : launch_latent_bwd<4, true>(p, st, parts, tiles, s);
      else rc = j2 ? launch_latent_bwd<2, false>(p, st, dz, ldz, s) : launch_latent_bwd<4, false>(p, st, dz, ldz, s);
      if (rc) return rc;
      break;
    }
    case LAT_DGRAD: {
      ProfScope ps(PC_OTHER, s, 2.0 * mbs * K2 * 8, 4.0 * mbs * K2);
      const int rpw = 8;
      const int nb = (mb + 4 * rpw - 1) / (4 * rpw);
      const int kq = K2 / 256;
#define IGI_LAT(KQ_) IGI_LAUNCH((k_latent_dgrad<KQ_, 8>), dim3(nb), dim3(256), 0, s, dz, ldz, w1p, p.xld, \
                                        p.obs, xcat, dxcat, mb, rpw)
      if (kq == 1) IGI_LAT(1); else if (kq == 2) IGI_LAT(2); else if (kq == 3) IGI_LAT(3); else IGI_LAT(4);
#undef IGI_LAT
      break;
    }
    case LAT_GENERIC: {
      GemmArgs g;
      g.A = dz; g.lda = ldz;
      g.B = w1p; g.ldb = p.xld;
      g.M = mb; g.N = p.xld; g.K = K2;
      g.C = dxcat; g.ldc = p.xld;
      g.aux = xcat; g.ldaux = p.xld;
      g.epilogue = EPI_TANHGRAD;
      IGI_HIP_TRY(gemm(g, true, false, s));
      break;
    }
  }
  if (p.ct_P > 0) {   // contact encoder backward from d(pre-tanh) of its columns of dxcat
    const hipError_t e = contact_backward(cta, s);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// backward through env_mlp (its last layer is already done when k_latent_bwd ran), then the closing group: the weight
// gradients still pending (the first env layer's, the first trunk layer's)
static int env_backward(const TeacherPlan& p, const StepPaths& q, const igi_teacher_state* st, PendingWgrads& pend,
                        hipStream_t s) {
  const float* P = st->params;
  const int mb = p.mb, pld = ru4(p.priv);
  float *priv_g = wsp<float>(st, p.w_priv), *xcat = wsp<float>(st, p.w_xcat), *dxcat = wsp<float>(st, p.w_dxcat);
  float* slab = wsp<float>(st, p.w_slab);
  for (int l = p.npl - 1 - p.lat_fused; l >= 0 && !p.ct_only; --l) {
    const int out = p.pu[l], in = env_in(p, l);
    const bool last = (l == p.npl - 1);
    const float* dz = last ? dxcat + p.obs : wsp<float>(st, p.w_de[l]);
    const int ldz = last ? p.xld : ru4(out);
    const float* x = (l == 0) ? priv_g : wsp<float>(st, p.w_e[l - 1]);
    const int ldx = (l == 0) ? pld : ru4(p.pu[l - 1]);
    if (l == 0 && p.lx_env) continue;   // done by the level above (LOWX)
    if (p.rb_env[l]) {
      RbLevelArgs r;
      r.dZ = dz; r.ldz = ldz;
      r.W = P + p.o_envW[l]; r.ldw = in;
      r.X = x; r.ldx = ldx;
      r.dX = wsp<float>(st, p.w_de[l - 1]); r.lddx = ru4(in);
      r.dWp = slab + p.s_envW[l]; r.ldwp = in; r.sWpart = (long long)out * in;
      r.dBp = slab + p.s_envB[l]; r.sBpart = out;
      r.rows = mb; r.IN = in; r.nets = 1; r.ranges = p.rb_env[l];
      if (p.lx_env && l == 1) {   // + the first env layer's weight / bias gradient; d(pre-activation) of that layer is not written
        r.lx_X = priv_g; r.lx_ld = pld;
        r.lx_W = slab + p.s_envW[0]; r.lx_ldw = env_in(p, 0); r.lx_sPart = (long long)p.pu[0] * env_in(p, 0);
        r.lx_B = slab + p.s_envB[0]; r.lx_bsPart = p.pu[0];
        if (q.latz) {
          // dZ of this layer is formed in the kernel from the latent row dots: it stages the layer's OUTPUT activations instead
          r.dZ = wsp<float>(st, p.w_e[1]); r.ldz = ru4(p.pu[1]);
          r.lz_parts = wsp<float>(st, p.w_lat_rowdot); r.lz_tiles = p.lat_tiles; r.lz_tstride = (long long)mb * 8;
          r.lz_lat = xcat + p.obs; r.lz_ldlat = p.xld;
          r.lz_W3 = P + p.o_envW[p.npl - 1];
          r.lz_rec = wsp<float>(st, p.w_lat_part); r.lz_srec = 8 * p.pu[1] + 8;
        }
      }
      const hipError_t e = rb_level_backward(r, s, PC_RB_ENV);
      if (e == hipErrorNotSupported) return IGI_E_UNSUPPORTED;
      IGI_HIP_TRY(e);
      continue;      // (weight gradients still pending -- the first trunk layer's -- go out with the last launch below)
    }
    {
      GemmArgs g;
      g.A = dz; g.lda = ldz;
      g.B = x; g.ldb = ldx;
      g.M = out; g.N = in; g.K = mb;
      g.C = slab + p.s_envW[l]; g.ldc = in;
      g.Cbias = slab + p.s_envB[l];
      g.splitk = p.sk_env[l];
      g.sCsplit = (long long)out * in; g.sCbiasSplit = out;
      pend.g[pend.n++] = g;
    }
    if (l > 0) {
      GemmArgs g;
      g.A = dz; g.lda = ldz;
      g.B = P + p.o_envW[l]; g.ldb = in;
      g.M = mb; g.N = in; g.K = out;
      g.C = wsp<float>(st, p.w_de[l - 1]); g.ldc = ru4(in);
      g.aux = wsp<float>(st, p.w_e[l - 1]); g.ldaux = ru4(in);
      g.epilogue = EPI_TANHGRAD;
      IGI_HIP_TRY(gemm_level(g, pend.g, pend.n, s, q.cls_env[l]));   // + this layer's (and the first trunk layer's) weight gradient
      pend.n = 0;
    }
  }
  IGI_HIP_TRY(gemm_wgrad_group(pend.g, pend.n, s, q.cls_closing));
  pend.n = 0;
  return 0;
}

// assemble the flat gradient: the segment table of this phase's partial sets, summed by k_slab_reduce
static int assemble_gradient(const TeacherPlan& p, const StepPaths& q, const igi_teacher_state* st, bool do0, bool do1,
                             hipStream_t s) {
  const int H = p.u[p.nl - 1];
  const float* slab = wsp<float>(st, p.w_slab);
  SegTable t;
  t.n = 0;
  bool seg_overflow = false;   // a table that is full refuses the step: nothing is ever written past s[MAX_SEG - 1]
  auto add = [&](long long dst, const float* src, long long stride, int rows, int cols, int src_ld,
                 int nparts) {
    if (t.n >= MAX_SEG) { seg_overflow = true; return; }
    Segment& sg = t.s[t.n++];
    sg.dst = dst; sg.src = src; sg.stride = stride; sg.count = rows * cols; sg.cols = cols;
    sg.src_ld = src_ld; sg.nparts = nparts;
  };
  const float* hs = wsp<float>(st, p.w_head_slab);
  const int hc = p.head_count;
  if (do0) {
    add(p.o_muW, hs, hc, 1, p.act * H, 0, p.loss_blocks);
    add(p.o_muB, hs + p.act * H, hc, 1, p.act, 0, p.loss_blocks);
    add(p.o_valW, hs + p.act * H + p.act, hc, 1, H, 0, p.loss_blocks);
    add(p.o_valB, hs + p.act * H + p.act + H, hc, 1, 1, 0, p.loss_blocks);
  }
  if (do1) add(p.o_sigma, hs + p.act * H + p.act + H + 1, hc, 1, p.act, 0, p.loss_blocks);
  for (int l = 0; l < p.npl - p.lat_fused && do1 && !p.ct_only; ++l) {
    const int out = p.pu[l], in = env_in(p, l);
    add(p.o_envW[l], slab + p.s_envW[l], (long long)out * in, 1, out * in, 0, p.sk_env[l]);
    add(p.o_envB[l], slab + p.s_envB[l], out, 1, out, 0, p.sk_env[l]);
  }
  if (p.lat_fused && do1) {
    const int H2 = p.pu[p.npl - 2], pc = 8 * H2 + 8;
    const float* part = wsp<float>(st, p.w_lat_part);
    const int nrec = q.latz ? p.rb_env[1] : p.lat_blocks;   // LATZ: one record per row range
    add(p.o_envW[p.npl - 1], part, pc, 1, 8 * H2, 0, nrec);
    add(p.o_envB[p.npl - 1], part + 8 * H2, pc, 1, 8, 0, nrec);
  }
  if (p.ct_P > 0 && do1) {   // encoder partial records [dW1 | db1 | dW2 | db2]; the decoder's slots are never written
    const float* part = wsp<float>(st, p.w_ct_part);
    const long long w1 = (long long)CT_HID * p.ct_P;
    add(p.o_ctW1, part, p.ct_rec, 1, (int)w1, 0, p.ct_blocks);
    add(p.o_ctB1, part + w1, p.ct_rec, 1, CT_HID, 0, p.ct_blocks);
    add(p.o_ctW2, part + w1 + CT_HID, p.ct_rec, 1, p.ct_E * CT_HID, 0, p.ct_blocks);
    add(p.o_ctB2, part + w1 + CT_HID + p.ct_E * CT_HID, p.ct_rec, 1, p.ct_E, 0, p.ct_blocks);
  }
  for (int l = 0; l < p.nl; ++l) {
    if (!(l > 0 ? do0 : do1)) continue;
    const int out = p.u[l], in = ac_in(p, l);
    const int inw = (l == 0) ? p.xld : in;  // slab rows are inw wide; the parameter rows are `in` wide
    for (int net = 0; net < p.nets; ++net) {
      add(p.o_acW[l] + net * p.ac_block, slab + p.s_acW[l] + (long long)net * out * inw,
          (long long)p.nets * out * inw, out, in, inw, p.sk_ac[l]);
      add(p.o_acB[l] + net * p.ac_block, slab + p.s_acB[l] + (long long)net * out, (long long)p.nets * out, 1, out, 0,
          p.sk_ac[l]);
    }
  }
  if (seg_overflow) return IGI_E_UNSUPPORTED;
  {
    ProfScope ps(PC_SLAB_REDUCE, s, 0.0, 4.0 * ((double)p.slab_floats + (double)hc * p.loss_blocks + p.P));
    // blocks per segment: 64 / 128 / 256 / 512 / 1024 / 2048 -> 29.5 / 19.2 / 15.4 / 14.3 / 15.0 / 17.9 us
    // (with the row-block levels' fewer, larger partial sets: 256 -> 13.0 us, 384 -> 13.9, 512 -> 14.2)
    IGI_LAUNCH(k_slab_reduce, dim3(SLAB_GX, t.n), dim3(RED_THREADS), 0, s, t, st->grads);
  }
  return (int)hipGetLastError();
}

// skip_gather: the previous step's fused tail (k_adam_gather) already gathered + normalised this minibatch
static int teacher_fwd_bwd(const igi_teacher_cfg* c, const igi_rollout* ro, const igi_teacher_state* st, int mb_index, int step_slot,
                           hipStream_t s, int phase = -1, bool skip_gather = false, const igi_kl_stop* ks = nullptr) {
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if ((rc = check_ks(ks, st, c))) return rc;
  if (!ro || !ro->obses || !ro->priv_info || !ro->actions || !ro->neglogpacs || !st->grads ||
      !st->perm || !st->rms_obs || !st->rms_priv || !st->stats || !st->advantages ||
      mb_index < 0 || mb_index >= p.nmb || step_slot < 0 || (p.ct_P > 0 && !ro->contacts))
    return IGI_E_BADARG;
  if (mb_index != step_slot % p.nmb || step_slot >= p.E * p.nmb) return IGI_E_BADARG;  // canonical step order
  if (phase < -1 || phase > 1) return IGI_E_BADARG;
  const bool do0 = phase != 1, do1 = phase != 0;
  // KL early stopping: what runs ahead of the step's decision looks at the word an EARLIER step left; step 0 has none
  // (the word still holds the previous update's result)
  const int32_t* stop = kl_stop_on(ks) && step_slot > 0 ? ks->stop_state : nullptr;
  const ContactArgs cta = p.ct_P > 0 ? contact_args(p, st, ro->contacts, st->perm, (long long)mb_index * p.mb, p.mb) : ContactArgs();
  // (from the plan and the state's addresses alone: phase 0 and phase 1 of a step resolve the same paths)
  const StepPaths q = resolve_paths(p, st);
  PendingWgrads pend;
  if (do0 && !skip_gather) gather_stage(p, ro, st, mb_index, step_slot, stop, s);
  // forward trunk (models_split.py:166-232), then heads + loss + head backward
  if (do0 && (rc = trunk_forward(p, st, p.mb, false, s, p.loss_fused ? p.nl - 1 : p.nl, p.ct_P > 0 ? &cta : nullptr))) return rc;
  if (do0 && (rc = loss_stage(p, c, ro, st, mb_index, dz_ld(p, p.nl - 1), dz_stride(p, p.nl - 1), s, stop))) return rc;
  if ((rc = trunk_backward(p, q, st, do0, do1, pend, s))) return rc;
  if (do1 && (rc = latent_backward(p, q, st, cta, s))) return rc;
  if (do1 && (rc = env_backward(p, q, st, pend, s))) return rc;
  return assemble_gradient(p, q, st, do0, do1, s);
}

// The scheduler launch behind the last optimizer step (step_slot) of a mini-epoch; the modes are k_lr_schedule's.
enum LrMode {
  LR_SINGLE = 0,  // one rank: mean and decision
  LR_BEGIN = 1,   // data parallel, ahead of the exchange: this rank's mini-epoch KL into the scratch float
  LR_END = 2,     // data parallel, behind it: the decision from the rank sum
};
static int teacher_lr_schedule(const igi_teacher_cfg* c, const TeacherPlan& p, const igi_teacher_state* st, int step_slot,
                               LrMode mode, int world, hipStream_t s, const int32_t* stop) {
  const int e = step_slot / p.nmb;
  if (e >= p.E || step_slot % p.nmb != p.nmb - 1) return IGI_E_BADARG;
  const float* rows = st->stats + (long long)e * p.nmb * IGI_STATS_PER_STEP;
  ProfScope ps(PC_LR_SCHEDULE, s, 0.0, 4.0 * p.nmb + 32.0);
  IGI_LAUNCH(k_lr_schedule, dim3(1), dim3(64), 0, s, rows, p.nmb, e, (int)mode, world, c->kl_threshold, c->lr_min, c->lr_max,
             st->lr_state, stop);
  return (int)hipGetLastError();
}

// next_ro != NULL: fuse the gather + normalise of optimizer step (next_mb, next_slot) into this step's Adam launch
// (k_sumsq_stats computes both norms and the statistics row first)
// x == NULL (one rank): with the adaptive schedule, run the scheduler when step_slot ends a mini-epoch.  x != NULL (data
// parallel): the stop decides on the rank mean of the estimator, exchanged here; the scheduler is left to
// teacher_update_steps, which puts the KL exchange between its two halves
static int teacher_apply(const igi_teacher_cfg* c, const igi_teacher_state* st, int step_slot,
                         int64_t adam_t, float grad_scale, hipStream_t s, const igi_rollout* next_ro = nullptr,
                         int next_mb = 0, int next_slot = 0, const igi_kl_stop* ks = nullptr,
                         const UpdateExchange* x = nullptr) {
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if ((rc = check_lr_cfg(c, st))) return rc;
  if ((rc = check_ks(ks, st, c))) return rc;
  const bool adaptive = lr_adaptive(c);
  int32_t* stop = kl_stop_on(ks) ? ks->stop_state : nullptr;
  if ((adaptive || stop) && (step_slot < 0 || step_slot >= p.E * p.nmb)) return IGI_E_BADARG;
  const bool sched = adaptive && !x && step_slot % p.nmb == p.nmb - 1;
  const bool exchanged = stop && x;
  if (!st->grads || !st->adam_m || !st->adam_v || adam_t < 1) return IGI_E_BADARG;
  double* part = wsp<double>(st, p.w_sumsq);
  float* row = st->stats ? st->stats + (long long)step_slot * IGI_STATS_PER_STEP : nullptr;
  {
    ProfScope ps(PC_SUMSQ, s, 0.0, 8.0 * (double)p.P);
    IGI_LAUNCH(k_sumsq_stats, dim3(SUMSQ_BLOCKS + (row ? 1 : 0)), dim3(256), 0, s, st->grads,
                       st->params, p.P, grad_scale, part, wsp<double>(st, p.w_loss_part), p.loss_blocks,
                       p.mb, row, StopArgs{stop, step_slot, stop ? 1.5 * ks->kl_threshold : 0.0, exchanged ? 1 : 0});
  }
  if (exchanged) {   // data parallel: the rank-mean estimator decides, between the norms and the Adam tail
    if (x->world < 1) return IGI_E_BADARG;
    if ((rc = exchange(x, XB_ESTIMATOR, step_slot))) return rc;
    ProfScope ps(PC_LR_SCHEDULE, s, 0.0, 16.0);
    IGI_LAUNCH(k_stop_decide, dim3(1), dim3(64), 0, s, stop, step_slot, x->world, 1.5 * ks->kl_threshold);
    if ((rc = (int)hipGetLastError())) return rc;
  }
  // torch.optim.Adam (_single_tensor_adam): python-double scalars, cast to fp32 at the tensor op
  const double b1 = c->beta1, b2 = c->beta2;
  const double bc1 = 1.0 - pow(b1, (double)adam_t);
  const double bc2 = 1.0 - pow(b2, (double)adam_t);
  const float step_size = (float)((double)c->lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const float w1 = (float)(1.0 - b1), w2 = (float)(1.0 - b2);
  int nb = (int)((p.P / 4 + 255) / 256);   // four elements per thread and trip
  if (nb > ADAM_BLOCKS_MAX) nb = ADAM_BLOCKS_MAX;
  if (nb < 1) nb = 1;
  if (next_ro) {
    if (!next_ro->obses || !next_ro->priv_info || !st->perm || !st->rms_obs || !st->rms_priv) return IGI_E_BADARG;
    const int D = p.obs + p.priv;
    ProfScope ps(PC_ADAM_GATHER, s, 0.0, 28.0 * (double)p.P + 8.0 * (double)p.mb * D + 8.0 * p.mb);
    AdamArgs aa;
    aa.params = st->params; aa.grads = st->grads; aa.m = st->adam_m; aa.v = st->adam_v; aa.P = p.P; aa.part = part;
    aa.scale = grad_scale; aa.max_norm = c->grad_norm; aa.w1 = w1; aa.beta2 = (float)b2; aa.w2 = w2;
    aa.step_size = step_size; aa.bc2_sqrt = bc2_sqrt; aa.eps = (float)c->adam_eps; aa.stats_row = row;
    aa.lr_dev = adaptive ? st->lr_state : nullptr; aa.bc1 = bc1; aa.stop = stop;
    GatherArgs ga = gather_args(p, next_ro, st, next_mb, next_slot);
    ga.stop = stop;   // the gather blocks of a stopping step must not publish step s + 1's running state
    W1Mirror mir;
    mir.w1p = ga.w1p; mir.wlat = ga.wlat; mir.o_w = ga.o_w; mir.ac_block = ga.ac_block; mir.u0 = ga.u0;
    mir.u0p = ga.u0p; mir.xw = p.xw; mir.xld = p.xld; mir.obs = p.obs; mir.K2p = ga.K2p; mir.nets = p.nets;
    IGI_LAUNCH(k_adam_gather, dim3(nb + p.gs_blocks), dim3(256), 0, s, aa, mir, ga, nb);
    if ((rc = (int)hipGetLastError())) return rc;
  } else {
    ProfScope ps(PC_ADAM, s, 0.0, 28.0 * (double)p.P);  // 16 B read + 12 B written per parameter
    IGI_LAUNCH(k_clip_adam, dim3(nb), dim3(256), 0, s, st->params, st->grads, st->adam_m,
                       st->adam_v, p.P, part, grad_scale, c->grad_norm, w1, (float)b2, w2, step_size,
                       bc2_sqrt, (float)c->adam_eps, row, 1.0f, 0.0f, adaptive ? st->lr_state : (const double*)nullptr, bc1,
                       (const int32_t*)stop);
    if ((rc = (int)hipGetLastError())) return rc;
  }
  return sched ? teacher_lr_schedule(c, p, st, step_slot, LR_SINGLE, 1, s, stop) : 0;
}

// KL early stopping, host side of the one-call updates: what reads the stop word while an update is being enqueued.
// One per device, owned by the library for the life of the process: a non-blocking copy stream, the events behind two
// consecutive mini-epochs, the event behind the copy, and the pinned word the copy lands in.  An update holds the
// device's reader -- its mutex -- from its first look-ahead to its last, so two host threads that update engines on one
// device take turns and never see each other's word.
struct StopReader {
  std::mutex use;
  hipStream_t cs = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr}, done = nullptr;
  int32_t* host = nullptr;
};
// built whole or not at all: a failure releases what it had created, and the next call starts afresh
static int stop_reader_build(StopReader& r) {
  hipStream_t cs = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int32_t* host = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(int32_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    for (int i = 0; i < 3; ++i)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (cs) (void)hipStreamDestroy(cs);
    return (int)e;
  }
  r.cs = cs; r.ev[0] = ev[0]; r.ev[1] = ev[1]; r.done = ev[2]; r.host = host;
  return 0;
}
// the calling thread's device's reader, locked; StopLookahead's destructor unlocks it
struct StopLookahead {
  StopReader* rd = nullptr;
  const igi_kl_stop* ks = nullptr;
  ~StopLookahead() { if (rd) rd->use.unlock(); }
  int begin(const igi_kl_stop* k) {
    static StopReader readers[64];
    int dev = 0;
    IGI_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return IGI_E_UNSUPPORTED;
    readers[dev].use.lock();
    rd = &readers[dev];
    ks = k;
    return rd->host ? 0 : stop_reader_build(*rd);
  }
  // behind mini-epoch e (enqueued on s, E in all): *stopped = the word as mini-epoch e - 1 left it says so
  int after_mini_epoch(int e, int E, hipStream_t s, bool* stopped) {
    *stopped = false;
    if (!rd || e + 1 >= E) return 0;
    IGI_HIP_TRY(hipEventRecord(rd->ev[e & 1], s));
    if (e < 1) return 0;
    IGI_HIP_TRY(hipStreamWaitEvent(rd->cs, rd->ev[(e - 1) & 1], 0));
    IGI_HIP_TRY(hipMemcpyAsync(rd->host, ks->stop_state, sizeof(int32_t), hipMemcpyDeviceToHost, rd->cs));
    IGI_HIP_TRY(hipEventRecord(rd->done, rd->cs));
    IGI_HIP_TRY(hipEventSynchronize(rd->done));
    *stopped = *rd->host >= 0;
    return 0;
  }
};

// The minibatch loop of the three one-call updates, p = make_plan(c): E mini-epochs x n_mb optimizer steps enqueued back
// to back on s (frozen_ppo.py:508-640).  x == NULL: one rank.  x != NULL: data parallel, the ranks' exchange goes
// through x between the stages of a step (the gradient exchange of :586-603, the KL float of :625-627), bucket by bucket.
// ks on: the device gates every step behind the stop on its own (exact at step granularity, no host involved); the
// host only stops ENQUEUEING, with one mini-epoch of look-ahead: mini-epoch e + 1 is in the queue before it waits for
// the event behind mini-epoch e and reads the word through the copy stream, which waits for that event alone -- never
// for the look-ahead work.  One host wait per mini-epoch; with the switch off there is none.  Data parallel, every
// rank reads the same word behind the same mini-epoch: all stop enqueueing at one boundary.
static int teacher_update_steps(const igi_teacher_cfg* c, const TeacherPlan& p, const igi_rollout* ro,
                                const igi_teacher_state* st, int64_t adam_t0, hipStream_t s, const igi_kl_stop* ks,
                                const UpdateExchange* x) {
  int rc;
  const int total = p.E * p.nmb;
  StopLookahead look;
  if (kl_stop_on(ks)) {
    if ((rc = check_state(p, st)) || (rc = check_ks(ks, st, c)) || (rc = look.begin(ks))) return rc;
  }
  const int32_t* stop = kl_stop_on(ks) ? ks->stop_state : nullptr;
  int slot = 0;
  for (int e = 0; e < p.E; ++e) {
    for (int i = 0; i < p.nmb; ++i, ++slot) {
      const bool gathered = slot > 0;   // by the previous step's fused tail
      if (x && x->two_phase) {
        if ((rc = teacher_fwd_bwd(c, ro, st, i, slot, s, 0, gathered, ks))) return rc;
        if ((rc = exchange(x, XB_EARLY, slot))) return rc;
        if ((rc = teacher_fwd_bwd(c, ro, st, i, slot, s, 1, false, ks))) return rc;
      } else {
        if ((rc = teacher_fwd_bwd(c, ro, st, i, slot, s, -1, gathered, ks))) return rc;
      }
      if (x && ((rc = exchange(x, XB_LATE, slot)) || (rc = exchange(x, XB_JOIN, slot)))) return rc;
      const bool more = slot + 1 < total;
      if ((rc = teacher_apply(c, st, slot, adam_t0 + slot + 1, x ? x->grad_scale : 1.0f, s, more ? ro : nullptr,
                              (slot + 1) % p.nmb, slot + 1, ks, x)))
        return rc;
      if (x && lr_adaptive(c) && i == p.nmb - 1) {
        // the rank-mean KL of the mini-epoch (frozen_ppo.py:625-627): every rank then takes the same decision
        if ((rc = teacher_lr_schedule(c, p, st, slot, LR_BEGIN, 1, s, stop))) return rc;
        if ((rc = exchange(x, XB_KL, slot))) return rc;
        if ((rc = teacher_lr_schedule(c, p, st, slot, LR_END, x->world, s, stop))) return rc;
      }
    }
    bool stopped;
    if ((rc = look.after_mini_epoch(e, p.E, s, &stopped))) return rc;
    if (stopped) break;
  }
  return 0;
}

static int teacher_update(const igi_teacher_cfg* c, const igi_rollout* ro,
                          const igi_teacher_state* st, int64_t adam_t0, hipStream_t s, const igi_kl_stop* ks = nullptr) {
  TeacherPlan p;
  const int rc = make_plan(c, &p);
  return rc ? rc : teacher_update_steps(c, p, ro, st, adam_t0, s, ks, nullptr);
}

// data-parallel update: the same steps with the two-bucket gradient exchange driven through a callback, which sees the
// buckets as they are; one host call per update, the callback only enqueues collectives / stream waits
static int teacher_update_dp(const igi_teacher_cfg* c, const igi_rollout* ro, const igi_teacher_state* st,
                             int64_t adam_t0, float grad_scale, igi_reduce_fn reduce, void* user, hipStream_t s,
                             const igi_kl_stop* ks = nullptr) {
  TeacherPlan p;
  const int rc = make_plan(c, &p);
  if (rc) return rc;
  const int world = grad_scale > 0.f ? (int)lroundf(1.0f / grad_scale) : 0;
  if ((lr_adaptive(c) || kl_stop_on(ks)) && world < 1) return IGI_E_BADARG;
  const UpdateExchange x{world, grad_scale, /*two_phase=*/true, /*foreign=*/true, user, reduce};
  return teacher_update_steps(c, p, ro, st, adam_t0, s, ks, &x);
}

static int teacher_infer(const igi_teacher_cfg* c, const igi_teacher_state* st, const float* obs,
                         const float* priv, int64_t rows, int normalize, float* mu, float* value,
                         float* latent, hipStream_t s, const float* contacts = nullptr) {
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if (!obs || !priv || rows < 0 || (normalize && (!st->rms_obs || !st->rms_priv))) return IGI_E_BADARG;
  if (p.ct_P > 0 && !contacts) return IGI_E_BADARG;
  const int lat_w = p.xw - p.obs;   // latent_gt: [priv latent | contact embedding] (models_split.py:172-177)
  float* priv_g = wsp<float>(st, p.w_priv);
  float* xcat = wsp<float>(st, p.w_xcat);
  float* ncoef = wsp<float>(st, p.w_norm_coef);
  const int pld = ru4(p.priv);
  const int D = p.obs + p.priv;
  const int H = p.u[p.nl - 1];
  const int ldh = ru4(H);
  if (normalize)
    IGI_LAUNCH(k_rms_coef, dim3(1), dim3(128), 0, s, p.obs, p.priv, st->rms_obs, st->rms_priv,
                       c->rms_eps, ncoef);
  for (int64_t r0 = 0; r0 < rows; r0 += p.mb) {
    const int nr = (int)((rows - r0 < p.mb) ? rows - r0 : p.mb);
    long long tot = (long long)nr * D;
    int nb = (int)((tot + 255) / 256);
    if (nb > 2048) nb = 2048;
    IGI_LAUNCH(k_copy_rows, dim3(nb), dim3(256), 0, s, obs + r0 * p.obs, priv + r0 * p.priv, nr,
                       p.obs, p.priv, xcat, p.xld, priv_g, pld);
    if (normalize)
      IGI_LAUNCH(k_normalize, dim3(nb), dim3(256), 0, s, xcat, p.xld, p.xw, priv_g, pld, nr, p.obs,
                         p.priv, ncoef);
    const ContactArgs cta = p.ct_P > 0 ? contact_args(p, st, contacts + r0 * p.ct_P, nullptr, 0, nr) : ContactArgs();
    if ((rc = trunk_forward(p, st, nr, true, s, -1, p.ct_P > 0 ? &cta : nullptr))) return rc;
    if (latent)
      IGI_HIP_TRY(hipMemcpy2DAsync(latent + r0 * lat_w, sizeof(float) * lat_w, xcat + p.obs,
                                   sizeof(float) * p.xld, sizeof(float) * lat_w, nr,
                                   hipMemcpyDeviceToDevice, s));
    if (mu || value) {
      const float* P = st->params;
      int hb = (nr + 3) / 4;
      if (hb > 1024) hb = 1024;
      const float* h = wsp<float>(st, p.w_h[p.nl - 1]);
      const long long ns = p.nets == 2 ? (long long)p.mb * ldh : 0;   // shared trunk: the value head reads the actor's rows
      float* mo = mu ? mu + r0 * p.act : nullptr;
      float* vo = value ? value + r0 : nullptr;
      IGI_LAUNCH_MAXJ(k_heads_infer, H, dim3(hb), dim3(256), 0, s, h, ns, ldh, H, P + p.o_muW, P + p.o_muB, P + p.o_valW,
                      P + p.o_valB, nr, p.act, mo, vo);
    }
  }
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Rollout-side policy step (frozen_ppo.py:343-366 + 655-665): ONE host call per environment step instead of
// igi_teacher_infer (10 launches) + a torch randn + igi_rollout_act_store.  With the reference's layer sizes and xcat
// no wider than 32 columns -- with or without contacts -- it is k_policy_stage + the persistent kernel of policy_fwd.h;
// every other shape takes 7-10 launches:
//   k_policy_stage   : raw obs / priv -> arena slot t (raw copies), normalised xcat / priv_g with the CURRENT running
//                      statistics (eval mode), zero padding, refresh of the padded first-layer weight
//   trunk_forward    : env_mlp + actor / critic trunk (the launches of the training forward)
//   k_heads_act_store: mu / value heads, action = mu + sigma * noise, neglogp, value de-normalisation, arena writes,
//                      clamp(action, +-1) for env.step
// Same arithmetic, in the same order, as the separate kernels (k_rms_coef + k_copy_rows + k_normalize, k_heads_infer,
// k_rollout_act_store): bit-identical outputs.
// ---------------------------------------------------------------------------------------------
struct PolicyStageArgs {
  const float* obs; const float* priv; int rows, obs_dim, priv_dim;
  const double* rms_obs; const double* rms_priv; float eps; int normalize;
  float* xcat; int xld, xw; float* priv_g; int pld;
  float* obses_t; float* priv_t;            // arena slot (raw copies) or NULL
  const float* params; long long o_w, ac_block; int u0, u0p; float* w1p;
  int stage_blocks, nets;
};

__global__ __launch_bounds__(256) void k_policy_stage(const PolicyStageArgs a) {
  if ((int)blockIdx.x >= a.stage_blocks) {  // W1p[net][o][c] refresh (see k_pad_w1)
    const int total = a.nets * a.u0p * a.xld;
    const int nb = (int)gridDim.x - a.stage_blocks;
    for (int e = ((int)blockIdx.x - a.stage_blocks) * blockDim.x + threadIdx.x; e < total; e += nb * blockDim.x) {
      const int c = e % a.xld;
      const int o = (e / a.xld) % a.u0p;
      const int net = e / (a.xld * a.u0p);
      a.w1p[e] = (c < a.xw && o < a.u0) ? a.params[a.o_w + net * a.ac_block + (long long)o * a.xw + c] : 0.f;
    }
    return;
  }
  const int D = a.obs_dim + a.priv_dim;
  const long long total = (long long)a.rows * D;
  const long long stride = (long long)a.stage_blocks * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long r = e / D;
    const int c = (int)(e - r * D);
    const bool is_obs = c < a.obs_dim;
    const int cc = is_obs ? c : c - a.obs_dim;
    const float x = is_obs ? a.obs[r * a.obs_dim + cc] : a.priv[r * a.priv_dim + cc];
    if (is_obs) { if (a.obses_t) a.obses_t[r * a.obs_dim + cc] = x; }
    else if (a.priv_t) a.priv_t[r * a.priv_dim + cc] = x;
    float y = x;
    if (a.normalize) {  // k_rms_coef + k_normalize: fp32 (mean, sqrt(var + eps)) from the fp64 running state
      const double* stt = is_obs ? a.rms_obs : a.rms_priv;
      const int d = is_obs ? a.obs_dim : a.priv_dim;
      const float m = (float)stt[cc], den = sqrtf((float)stt[d + cc] + a.eps);
      y = clamp5((x - m) / den);
    }
    if (is_obs) a.xcat[r * a.xld + cc] = y;
    else a.priv_g[r * a.pld + cc] = y;
  }
  const int padw = a.xld - a.xw;   // keep the zero padding of xcat zero (feeds the padded first layer)
  const long long ptotal = (long long)a.rows * padw;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ptotal; e += stride) {
    const long long r = e / padw;
    a.xcat[r * a.xld + a.xw + (int)(e - r * padw)] = 0.f;
  }
}

struct ActStoreArgs {
  const float* logstd; const float* noise; const double* rms_value; float eps;
  float* actions_t; float* nlp_t; float* values_t; float* mus_t; float* sigmas_t; float* actions_clamped;
  float* values_out;
};

// one wave per row: the heads as k_heads_infer computes them (head_products_row), then lane q owns action q
template <int MAXJ>
__global__ __launch_bounds__(256) void k_heads_act_store(const float* __restrict__ h, long long net_stride, int ldh,
                                                         int H, const float* __restrict__ Wmu,
                                                         const float* __restrict__ bmu, const float* __restrict__ Wv,
                                                         const float* __restrict__ bv, int rows, int act,
                                                         const ActStoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nw = (gridDim.x * blockDim.x) >> 6;
  float vm = 0.f, vd = 1.f;
  if (a.rms_value) { vm = (float)a.rms_value[0]; vd = sqrtf((float)a.rms_value[1] + a.eps); }
  const float my_logstd = lane < act ? a.logstd[lane] : 0.f;
  const float my_bmu = lane < act ? bmu[lane] : 0.f;
  for (int row = gw; row < rows; row += nw) {
    const float* ha_p = h + (long long)row * ldh;
    float pm[IGI_MAX_ACT], pv;
    head_products_row<MAXJ>(ha_p, ha_p + net_stride, H, Wmu, Wv, act, lane, pm, pv);
    pv = wave_sum(pv);
    float my_pm = 0.f;
#pragma unroll
    for (int q = 0; q < IGI_MAX_ACT; ++q)
      if (q < act) { const float t = wave_sum(pm[q]); my_pm = (lane == q) ? t : my_pm; }
    // per-action arithmetic of k_rollout_act_store on lane q
    const float m = my_pm + my_bmu;
    const float sig = expf(m * 0.f + my_logstd);
    const long long ia = (long long)row * act + lane;
    const float nz = lane < act ? a.noise[ia] : 0.f;
    const float av = m + sig * nz;
    const float x = av - m;
    const float term = ((x * x) / (2.0f * (sig * sig)) + logf(sig)) + ROLL_LOG_SQRT_2PI;
    if (lane < act) {
      a.actions_t[ia] = av;
      a.mus_t[ia] = m;
      a.sigmas_t[ia] = sig;
      a.actions_clamped[ia] = fminf(fmaxf(av, -1.0f), 1.0f);
    }
    float nlp = 0.f;   // summed in action order, as the one-thread-per-env kernel does
    for (int q = 0; q < act; ++q) nlp += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term), q));
    if (lane == 0) {
      float v = pv + bv[0];
      if (a.rms_value) v = vd * fminf(fmaxf(v, -5.0f), 5.0f) + vm;
      a.nlp_t[row] = nlp;
      a.values_t[row] = v;
      a.values_out[row] = v;
    }
  }
}

static int teacher_policy_step(const igi_teacher_cfg* c, const igi_teacher_state* st, const float* obs,
                               const float* priv, int64_t rows, int normalize, const float* noise,
                               const double* rms_value, float* obses_t, float* priv_t, float* actions_t, float* nlp_t,
                               float* values_t, float* mus_t, float* sigmas_t, float* actions_clamped,
                               float* values_out, hipStream_t s, const float* contacts = nullptr,
                               float* contacts_t = nullptr) {   // contacts_t: slot t of the (T, N, P) arena, may be NULL
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if (!obs || !priv || rows < 1 || !noise || !actions_t || !nlp_t || !values_t || !mus_t || !sigmas_t ||
      !actions_clamped || !values_out || (normalize && (!st->rms_obs || !st->rms_priv)))
    return IGI_E_BADARG;
  if (p.act > 64) return IGI_E_UNSUPPORTED;
  if (p.ct_P > 0 && !contacts) return IGI_E_BADARG;
  const float* P = st->params;
  const int H = p.u[p.nl - 1];
  const int ldh = ru4(H);
  const int D = p.obs + p.priv;
  for (int64_t r0 = 0; r0 < rows; r0 += p.mb) {
    const int nr = (int)((rows - r0 < p.mb) ? rows - r0 : p.mb);
    PolicyStageArgs a;
    a.obs = obs + r0 * p.obs; a.priv = priv + r0 * p.priv; a.rows = nr; a.obs_dim = p.obs; a.priv_dim = p.priv;
    a.rms_obs = st->rms_obs; a.rms_priv = st->rms_priv; a.eps = c->rms_eps; a.normalize = normalize;
    a.xcat = wsp<float>(st, p.w_xcat); a.xld = p.xld; a.xw = p.xw; a.priv_g = wsp<float>(st, p.w_priv);
    a.pld = ru4(p.priv);
    a.obses_t = obses_t ? obses_t + r0 * p.obs : nullptr; a.priv_t = priv_t ? priv_t + r0 * p.priv : nullptr;
    a.params = P; a.o_w = p.o_acW[0]; a.ac_block = p.ac_block; a.u0 = p.u[0]; a.u0p = p.u0p;
    a.w1p = wsp<float>(st, p.w_w1p);
    long long tot = (long long)nr * D;
    int nb = (int)((tot + 255) / 256);
    if (nb > 2048) nb = 2048;
    a.stage_blocks = nb; a.nets = p.nets;
    const int pad_blocks = 16;
    {
      ProfScope ps(PC_OTHER, s, 0.0, 8.0 * tot);
      IGI_LAUNCH(k_policy_stage, dim3(nb + pad_blocks), dim3(256), 0, s, a);
    }
    // (the persistent kernel assigns one net per workgroup pair: a shared trunk takes the per-layer launches)
    if (p.nets == 2 && !bf16_mode() && policy_fwd_shape_ok(p.obs, p.priv, p.act, p.npl, p.pu, p.nl, p.u, p.xw) && p.xld == 32) {
      // env_mlp, the contact encoder, both trunks, the heads, the sample and the arena writes (the step's raw contacts
      // among them) of these rows as ONE persistent launch (policy_fwd.h)
      PolicyFwdArgs f;
      if (p.ct_P > 0) {
        f.ct = contacts + r0 * p.ct_P; f.ct_t = contacts_t ? contacts_t + r0 * p.ct_P : nullptr; f.ctP = p.ct_P; f.ctE = p.ct_E;
        f.cW1 = P + p.o_ctW1; f.cb1 = P + p.o_ctB1; f.cW2 = P + p.o_ctW2; f.cb2 = P + p.o_ctB2;
      }
      f.xw = p.xw;
      f.priv = a.priv_g; f.ldp = a.pld; f.xcat = a.xcat; f.ldx = p.xld; f.rows = nr; f.obs = p.obs; f.act = p.act;
      f.eW1 = P + p.o_envW[0]; f.eb1 = P + p.o_envB[0]; f.eW2 = P + p.o_envW[1]; f.eb2 = P + p.o_envB[1];
      f.eW3 = P + p.o_envW[2]; f.eb3 = P + p.o_envB[2];
      f.w1p = a.w1p; f.tb1 = P + p.o_acB[0]; f.tW2 = P + p.o_acW[1]; f.tb2 = P + p.o_acB[1]; f.tW3 = P + p.o_acW[2];
      f.tb3 = P + p.o_acB[2]; f.ac_block = p.ac_block;
      f.Wmu = P + p.o_muW; f.bmu = P + p.o_muB; f.Wv = P + p.o_valW; f.bv = P + p.o_valB; f.logstd = P + p.o_sigma;
      f.noise = noise + r0 * p.act; f.rms_value = rms_value; f.eps = c->rms_eps;
      f.actions_t = actions_t + r0 * p.act; f.nlp_t = nlp_t + r0; f.values_t = values_t + r0;
      f.mus_t = mus_t + r0 * p.act; f.sigmas_t = sigmas_t + r0 * p.act;
      f.actions_clamped = actions_clamped + r0 * p.act; f.values_out = values_out + r0;
      const hipError_t e = policy_forward(f, s, p.ct_P == 0 ? PF_NO_CONTACTS : p.ct_only ? PF_ONLY_CONTACT : PF_CONTACTS);
      if (e == hipSuccess) continue;
      if (e != hipErrorInvalidValue) return (int)e;      // (alignment of the caller's buffers: the per-layer launches below)
    }
    const ContactArgs cta = p.ct_P > 0 ? contact_args(p, st, contacts + r0 * p.ct_P, nullptr, 0, nr) : ContactArgs();
    if ((rc = trunk_forward(p, st, nr, false, s, -1, p.ct_P > 0 ? &cta : nullptr))) return rc;
    if (p.ct_P > 0 && contacts_t)   // the arena write of this step's contacts (frozen_ppo.py:663-664), raw
      IGI_HIP_TRY(hipMemcpyAsync(contacts_t + r0 * p.ct_P, contacts + r0 * p.ct_P, sizeof(float) * nr * p.ct_P,
                                 hipMemcpyDeviceToDevice, s));
    ActStoreArgs t;
    t.logstd = P + p.o_sigma; t.noise = noise + r0 * p.act; t.rms_value = rms_value; t.eps = c->rms_eps;
    t.actions_t = actions_t + r0 * p.act; t.nlp_t = nlp_t + r0; t.values_t = values_t + r0;
    t.mus_t = mus_t + r0 * p.act; t.sigmas_t = sigmas_t + r0 * p.act;
    t.actions_clamped = actions_clamped + r0 * p.act; t.values_out = values_out + r0;
    int hb = (nr + 3) / 4;
    if (hb > 1024) hb = 1024;
    const float* h = wsp<float>(st, p.w_h[p.nl - 1]);
    const long long ns = p.nets == 2 ? (long long)p.mb * ldh : 0;
    ProfScope ps(PC_OTHER, s, 0.0, 8.0 * nr * H);
    IGI_LAUNCH_MAXJ(k_heads_act_store, H, dim3(hb), dim3(256), 0, s, h, ns, ldh, H, P + p.o_muW, P + p.o_muB, P + p.o_valW,
                    P + p.o_valB, nr, p.act, t);
  }
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The frozen ACTOR on [obs | student latent] (ActorCriticSplit.act_inference / act_with_grad with a `latent` entry:
// ext_adapt.py:684-690 in the stage-2 rollout, :799-806 in the student's update, deploy_s2): mu only -- the value those
// callers throw away is not computed -- and the data gradient of a loss on mu back into the latent.  The teacher's
// weights are constants here: no weight gradient.
//   forward : k_pad_w1 + ONE k_actor_latent launch per chunk of mb rows (policy_fwd.h) at the reference's layer sizes;
//             every other shape: k_stage_obs_latent, the actor's Linear + Tanh layers (gemm, nbatch = 1), k_heads_infer.
//             hsave (may be NULL): [rows][S], S = sum of ru4(u_l): the post-tanh activations, layer l at column
//             offset sum of ru4(u_k), k < l -- the caller's tensor, because the backward pass runs later.
//   backward: dZ_l = (dZ_{l+1} . W_{l+1}) * (1 - h_l^2) from dZ_{nl} = dmu and W_{nl} = Wmu, then
//             dlatent = dZ_0 . W_0[:, obs : obs + L].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stage_obs_latent(const float* __restrict__ obs_n, const float* __restrict__ latent,
                                                          int rows, int obs, int L, float* __restrict__ xcat, int xld) {
  const long long total = (long long)rows * xld;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long r = e / xld;
    const int c = (int)(e - r * xld);
    xcat[e] = c < obs ? obs_n[r * obs + c] : (c < obs + L ? latent[r * L + (c - obs)] : 0.f);
  }
}

static inline int actor_latent_saved_width(const TeacherPlan& p) {
  int w = 0;
  for (int l = 0; l < p.nl; ++l) w += ru4(p.u[l]);
  return w;
}

static int teacher_actor_latent_forward(const igi_teacher_cfg* c, const igi_teacher_state* st, const float* obs_n,
                                        const float* latent, int L, int64_t rows, float* mu, float* hsave, hipStream_t s) {
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if (!obs_n || !latent || !mu || rows < 1 || L != p.xw - p.obs) return IGI_E_BADARG;
  const float* P = st->params;
  float* w1p = wsp<float>(st, p.w_w1p);
  float* xcat = wsp<float>(st, p.w_xcat);
  const int S = actor_latent_saved_width(p);
  const int H = p.u[p.nl - 1];
  {
    ProfScope ps(PC_OTHER, s, 0.0, 8.0 * p.nets * p.u0p * p.xld);
    IGI_LAUNCH(k_pad_w1, dim3((p.nets * p.u0p * p.xld + 255) / 256), dim3(256), 0, s, P, p.o_acW[0], p.ac_block, p.u[0],
               p.u0p, p.xw, p.xld, w1p, p.nets);
  }
  // (no nets == 2 term: the kernel runs the actor alone, a shared trunk's included)
  const bool fused = !bf16_mode() && actor_latent_shape_ok(p.obs, L, p.act, p.nl, p.u) && p.xld == 32;
  for (int64_t r0 = 0; r0 < rows; r0 += p.mb) {
    const int nr = (int)((rows - r0 < p.mb) ? rows - r0 : p.mb);
    float* hs = hsave ? hsave + r0 * S : nullptr;
    if (fused) {
      ActorLatentArgs f;
      f.obs_n = obs_n + r0 * p.obs; f.latent = latent + r0 * L; f.rows = nr; f.obs = p.obs; f.L = L; f.act = p.act;
      f.w1p = w1p; f.tb1 = P + p.o_acB[0]; f.tW2 = P + p.o_acW[1]; f.tb2 = P + p.o_acB[1]; f.tW3 = P + p.o_acW[2];
      f.tb3 = P + p.o_acB[2]; f.Wmu = P + p.o_muW; f.bmu = P + p.o_muB;
      f.mu = mu + r0 * p.act;
      if (hs) { f.h1 = hs; f.h2 = hs + ru4(p.u[0]); f.h3 = hs + ru4(p.u[0]) + ru4(p.u[1]); f.ldh = S; }
      const hipError_t e = actor_latent_forward(f, s);
      if (e == hipSuccess) continue;
      if (e != hipErrorInvalidValue) return (int)e;      // (alignment of the parameter vector: the per-layer launches below)
    }
    {
      const long long tot = (long long)nr * p.xld;
      int nb = (int)((tot + 255) / 256);
      if (nb > 2048) nb = 2048;
      ProfScope ps(PC_OTHER, s, 0.0, 8.0 * tot);
      IGI_LAUNCH(k_stage_obs_latent, dim3(nb), dim3(256), 0, s, obs_n + r0 * p.obs, latent + r0 * L, nr, p.obs, L, xcat, p.xld);
    }
    const float* in = xcat;
    int ldin = p.xld, col = 0;
    for (int l = 0; l < p.nl; ++l) {
      GemmArgs g;
      g.A = in; g.lda = ldin;
      if (l == 0) { g.B = w1p; g.ldb = p.xld; g.K = p.xld; g.flop_credit = (double)p.xw / p.xld; }
      else { g.B = P + p.o_acW[l]; g.ldb = ac_in(p, l); g.K = ac_in(p, l); }
      g.bias = P + p.o_acB[l];
      g.M = nr; g.N = p.u[l];
      if (hs) { g.C = hs + col; g.ldc = S; }
      else { g.C = wsp<float>(st, p.w_h[l]); g.ldc = ru4(p.u[l]); }
      g.epilogue = EPI_BIAS_TANH;
      IGI_HIP_TRY(gemm(g, true, true, s));
      in = g.C; ldin = g.ldc; col += ru4(p.u[l]);
    }
    int hb = (nr + 3) / 4;
    if (hb > 1024) hb = 1024;
    ProfScope ps(PC_OTHER, s, 0.0, 4.0 * nr * H);
    IGI_LAUNCH_MAXJ(k_heads_infer, H, dim3(hb), dim3(256), 0, s, in, 0LL, ldin, H, P + p.o_muW, P + p.o_muB, P + p.o_valW,
                    P + p.o_valB, nr, p.act, mu + r0 * p.act, (float*)nullptr);
  }
  return (int)hipGetLastError();
}

static int teacher_actor_latent_backward(const igi_teacher_cfg* c, const igi_teacher_state* st, const float* hsave,
                                         const float* dmu, int64_t rows, float* dlatent, hipStream_t s) {
  TeacherPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  if ((rc = check_state(p, st))) return rc;
  if (!hsave || !dmu || !dlatent || rows < 1) return IGI_E_BADARG;
  const float* P = st->params;
  const int L = p.xw - p.obs;
  const int S = actor_latent_saved_width(p);
  int off[IGI_MAX_LAYERS];
  for (int l = 0, col = 0; l < p.nl; ++l) { off[l] = col; col += ru4(p.u[l]); }
  for (int64_t r0 = 0; r0 < rows; r0 += p.mb) {
    const int nr = (int)((rows - r0 < p.mb) ? rows - r0 : p.mb);
    const float* hs = hsave + r0 * S;
    for (int l = p.nl - 1; l >= 0; --l) {       // dZ_l into the workspace's dh slot of layer l, rows ru4(u_l) floats apart
      GemmArgs g;
      if (l == p.nl - 1) { g.A = dmu + r0 * p.act; g.lda = p.act; g.B = P + p.o_muW; g.K = p.act; }
      else { g.A = wsp<float>(st, p.w_dh[l + 1]); g.lda = ru4(p.u[l + 1]); g.B = P + p.o_acW[l + 1]; g.K = p.u[l + 1]; }
      g.ldb = p.u[l];
      g.M = nr; g.N = p.u[l];
      g.C = wsp<float>(st, p.w_dh[l]); g.ldc = ru4(p.u[l]);
      g.aux = hs + off[l]; g.ldaux = S;
      g.epilogue = EPI_TANHGRAD;
      IGI_HIP_TRY(gemm(g, true, false, s));
    }
    const float* dz = wsp<float>(st, p.w_dh[0]);
    float* out = dlatent + r0 * L;
    if (L == 8 && p.u[0] % 256 == 0 && p.u[0] <= 1024) {
      ProfScope ps(PC_OTHER, s, 2.0 * nr * p.u[0] * 8, 4.0 * nr * p.u[0]);
      const int rpw = 8;
      const int nb = (nr + 4 * rpw - 1) / (4 * rpw);
      const int kq = p.u[0] / 256;
#define IGI_LATR(KQ_) IGI_LAUNCH((k_latent_dgrad<KQ_, 8, true>), dim3(nb), dim3(256), 0, s, dz, p.u0p, P + p.o_acW[0], p.xw, \
                                 p.obs, (const float*)nullptr, out, nr, rpw)
      if (kq == 1) IGI_LATR(1); else if (kq == 2) IGI_LATR(2); else if (kq == 3) IGI_LATR(3); else IGI_LATR(4);
#undef IGI_LATR
    } else {
      GemmArgs g;
      g.A = dz; g.lda = p.u0p;
      g.B = P + p.o_acW[0] + p.obs; g.ldb = p.xw;
      g.M = nr; g.N = L; g.K = p.u[0];
      g.C = out; g.ldc = L;
      g.epilogue = EPI_STORE;
      IGI_HIP_TRY(gemm(g, true, false, s));
    }
  }
  return (int)hipGetLastError();
}

}  // namespace igi
