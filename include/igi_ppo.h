/*
 * igi_ppo.h -- C ABI of libigi_hip.so: the MI355X (gfx950) learning-side hot path of
 * osheraz/IsaacGymInsertion (teacher PPO update).
 *
 * The reference has no FFI for this path: the boundary it exposes is the Python class API
 * (algo/ppo/frozen_ppo.py::PPO, algo/ppo/experience.py::ExperienceBuffer,
 * algo/models/models_split.py::ActorCriticSplit, algo/models/running_mean_std.py::RunningMeanStd).
 * Each entry point below replaces the chain of ATen ops behind one of those methods; the
 * citation on each declaration names the reference lines it replaces (paths relative to the
 * reference root).  isaacgyminsertion_amd/ binds these with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - no entry point allocates, frees, retains or synchronises: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream), memory is owned by the caller;
 *   - return value: 0 on success, a positive hipError_t, or a negative IGI_E_* code;
 *     igi_last_error() returns a static string describing the last failure on this thread;
 *   - all arithmetic is fp32 (exact-fp32 MFMA, v_mfma_f32_32x32x2_f32) except normaliser state
 *     and reductions feeding it, which are fp64 as in running_mean_std.py:44-46.
 */
#ifndef IGI_PPO_H
#define IGI_PPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGI_ABI_VERSION 6
#define IGI_MAX_LAYERS 4
#define IGI_MAX_ACT 8

#define IGI_E_BADARG (-1)
#define IGI_E_WORKSPACE (-2)
#define IGI_E_CALLBACK (-5)
#define IGI_E_UNSUPPORTED (-3)
#define IGI_E_COMM (-6)        /* an RCCL call failed: igi_comm_last_error() has the text */

typedef void* igi_stream_t;

int igi_abi_version(void);
/* sha256 prefix (32 hex digits) of the sources this library was compiled from (__graft_entry__.source_hash) */
const char* igi_build_info(void);
const char* igi_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Measurement hook (new; the reference only has wall-clock accumulators, frozen_ppo.py:272-274,
 * 500, 645).  After igi_prof_enable(1) every kernel launch of this library is bracketed by HIP
 * events on its own stream; igi_prof_read synchronises those events and returns one entry per
 * kernel class with the number of launches, their summed duration and the ALGORITHMIC flops /
 * bytes of those launches (SURVEY.md section 8d conventions).  igi_prof_enable(0|1) resets.
 * ---------------------------------------------------------------------------------------- */
typedef struct igi_prof_entry {
  const char* name;
  int64_t launches;
  double total_ms;
  double flops;
  double bytes;
} igi_prof_entry;
int igi_prof_enable(int on);
int igi_prof_read(igi_prof_entry* out_host, int max_entries);
/* The box's own fp32 matrix rate, measured ("re-measure on the box with a microbench and state
 * both"; the reference has no counterpart): one launch of `blocks` x 256 threads, each wave issuing iters x 16
 * MFMAs from registers only (no LDS, no memory) on non-trivial operands; shape 0 = v_mfma_f32_32x32x2_f32 (4096 flop
 * each: the instruction every fp32 product here runs on), 1 = v_mfma_f32_16x16x4_f32 (2048), 2 = v_mfma_f32_32x32x16_bf16
 * (32768) -> flops per launch = blocks * 4 * iters * 16 * flop; the caller times the launch.  clocks_dev (device, 2 * blocks uint64): per block the shader
 * cycles and the 100 MHz real-time ticks its first wave spent in the loop (clock = cycles / ticks * 100 MHz);
 * sink_dev: one device float that is never written in practice (keeps the loop alive). */
int igi_mfma_peak_probe(int shape, int blocks, int iters, uint64_t* clocks_dev, float* sink_dev, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Generic exact-fp32 MFMA GEMM used by every Linear forward / dgrad / wgrad on the path.
 *   C[m][n] (+)= sum_k A(m,k) * B(n,k)
 *   a_kcontig: A(m,k) = A[m*lda + k]  else A[k*lda + m];   b_kcontig likewise for B(n,k).
 * epilogue: 0 store | 1 tanh(acc + bias[n]) | 2 acc * (1 - aux[m][n]^2) | 3 acc + bias[n]
 *           4 relu(acc + bias[n]) | 5 acc * (aux[m][n] > 0)
 *           6 elu(acc + bias[n]) | 7 acc * elu'(.) with aux = the ELU OUTPUT (a > 0 ? 1 : a + 1)   [alpha = 1]
 * accumulate != 0 adds the previous contents of C before the epilogue.
 * Replaces torch.nn.Linear + nn.Tanh forward and their autograd backward
 * (algo/models/models_split.py:27-38, 222-228).
 * ---------------------------------------------------------------------------------------- */
/* Opt-in reduced-precision mode of the large Linear products (forward, data gradient and grouped weight gradient
 * of the 128-wide tiles): operands are rounded to bf16 (nearest even) as they are fed to v_mfma_f32_32x32x16_bf16,
 * accumulation stays fp32.  16x the matrix rate, ~3 significant digits per product -- NOT reference arithmetic:
 * off by default (also settable with IGI_GEMM_BF16=1), parity tests and the headline benchmark run with it off.
 * Returns the previous setting. */
int igi_gemm_set_bf16_inputs(int on);
/* The same opt-in mode for the three convolutions of the tactile encoder (igi_tactile_forward / igi_tactile_backward:
 * forward, data gradient and weight gradient of every layer, on every tile the encoder launches).  Each product term
 * is float(bf16(a)) * float(bf16(w)) -- exact in fp32 -- accumulated in fp32: the operands are rounded (nearest even)
 * where they are fed to v_mfma_f32_32x32x16_bf16; activations, pre-activation gradients, repacked weights and split-K
 * slabs stay fp32 in memory, and the loaders, the epilogues (bias + ReLU, ReLU', bias-gradient sums, soft-argmax
 * partials), the soft-argmax kernels, the 128 -> latent Linear and the fixed-order slab reduction are unchanged: two
 * runs are bit-identical.  Off by default; IGI_CONV_BF16=1 in the environment starts it on.  Independent of
 * igi_gemm_set_bf16_inputs: that switch never applies to a convolution, this one to nothing else (PointNet, the depth
 * backbone, the token encoder, every Linear and the teacher stay fp32).  igi_tactile_backward uses the setting in force
 * when IT is called: a forward / backward pair must run under ONE setting (the Python op's autograd formula records the
 * forward's setting and re-establishes it around the backward).  on < 0 only queries.  Returns the previous setting. */
int igi_conv_set_bf16_inputs(int on);
/* Opt-in split-bf16 mode of the same three convolutions (forward, data gradient and weight gradient of every layer, on
 * every tile the encoder launches): fp32-grade results from the bf16 matrix pipe.  Every operand element is split where
 * the MFMA operands are formed into three bf16 planes, x = hi + mid + lo (hi = bf16(x), mid = bf16(x - hi),
 * lo = bf16(x - hi - mid): three nearest-even conversions, two exact fp32 differences; exact for 2^-103 <= |x| <= the
 * largest bf16, and for 0), and every product term is the sum of the six plane products mid*mid, lo*hi, hi*lo, mid*hi,
 * hi*mid, hi*hi -- issued in that order inside each 16-k step, each exact in fp32, accumulated in fp32 on
 * v_mfma_f32_32x32x16_bf16; mid*lo, lo*mid and lo*lo, below 2^-24 of the leading product, are dropped.  Operands stay fp32
 * in memory; tiles, launch count, loaders, epilogues, the soft-argmax kernels, the 128 -> latent Linear and the split-K
 * reductions are the fp32 path's; two runs are bit-identical.  Off by default; IGI_CONV_BF16X3=1 in the environment
 * starts it on.  A switch of its own: igi_conv_set_bf16_inputs, igi_gemm_set_bf16_inputs, igi_gemm_set_bf16x3 and
 * igi_depth_set_bf16_inputs neither set it nor are set by it, and it reaches nothing but the tactile convolutions.  With
 * this switch and igi_conv_set_bf16_inputs BOTH on, igi_tactile_forward and igi_tactile_backward return IGI_E_BADARG.
 * A forward / backward pair must run under ONE setting, as above.  on < 0 only queries.  Returns the previous setting. */
int igi_conv_set_bf16x3(int on);
/* The same opt-in mode for the six large products of the depth backbone (igi_depth_forward / igi_depth_backward): conv2
 * (3 x 3, 32 -> 64) forward, data gradient and weight gradient, and the 64768 -> 128 Linear forward (split-K), data
 * gradient (with its ELU' epilogue) and weight gradient.  Each product term is float(bf16(a)) * float(bf16(b)), round to
 * nearest even, exact in fp32, accumulated in fp32 on v_mfma_f32_32x32x16_bf16; operands stay fp32 in memory and are
 * rounded where the MFMA operands are formed; the tiles are the fp32 path's.  Unchanged fp32: conv1 + max-pool + ELU with
 * its arg-max bytes (the mode changes no pool decision) and conv1's weight gradient, the 128 -> latent Linear, biases,
 * bias-gradient sums, ELU and ELU', the split-K reductions, the weight pack / permute kernels.  Deterministic.  Off by
 * default; IGI_DEPTH_BF16=1 in the environment starts it on.  Independent of igi_gemm_set_bf16_inputs and
 * igi_conv_set_bf16_inputs: neither reaches these six products' choice here, and this switch reaches nothing outside the
 * depth backbone.  igi_depth_backward must run under the setting its igi_depth_forward ran under (the autograd formula of
 * ops.depth_backbone_fwd records it and re-establishes it).  on < 0 only queries.  Returns the previous setting. */
int igi_depth_set_bf16_inputs(int on);
/* EXPERIMENT, off by default (IGI_GEMM_X3 = 6 | 9 in the environment starts it on): fp32 products on the bf16 matrix pipe by
 * an exact three-plane split of every operand element (x = hi + mid + lo in bf16: each plane product is exact in fp32, the
 * MFMA accumulates in fp32) for the large k-contiguous forward products (K >= 256).  products = 9: all nine cross products,
 * nothing dropped; 6: without mid*lo, lo*mid, lo*lo (each below 2^-24 of the leading product); 0: off.  Returns the previous
 * setting.  Not the arithmetic of the headline number: bench.py reports it beside it. */
int igi_gemm_set_bf16x3(int products);

int igi_gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K,
                 const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 const float* bias, const float* aux, int ldaux, int epilogue, int accumulate,
                 igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Running mean / std  (algo/models/running_mean_std.py:23-93).
 * state = [mean[D], var[D], count] as D+D+1 doubles.  train != 0: merge the batch moments of
 * x (rows x D, unbiased variance) into state first (Chan), then y = clamp((x-mean)/sqrt(var+eps),
 * +-5); unnorm != 0: y = sqrt(var+eps)*clamp(x,+-5)+mean (no update).
 * workspace: igi_rms_workspace_bytes(rows, D).
 * ---------------------------------------------------------------------------------------- */
size_t igi_rms_workspace_bytes(int64_t rows, int D);
int igi_rms_forward(const float* x, float* y, int64_t rows, int D, double* state, float eps,
                    int train, int unnorm, void* workspace, size_t workspace_bytes,
                    igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Teacher PPO update (algo/ppo/frozen_ppo.py:495-646, 714-725; algo/ppo/experience.py:199-263).
 * ---------------------------------------------------------------------------------------- */
typedef struct igi_teacher_cfg {
  int32_t obs_dim, priv_dim, act_dim;
  int32_t n_priv_layers;
  int32_t priv_units[IGI_MAX_LAYERS]; /* env_mlp widths; last = latent (models_split.py:73-76) */
  int32_t n_layers;
  int32_t units[IGI_MAX_LAYERS];      /* actor_mlp / critic_mlp widths (models_split.py:100-102) */
  int32_t num_envs, horizon, mini_epochs; /* N, T, E; minibatch = N*T/E (frozen_ppo.py:213-215) */
  int32_t shared_parameters;          /* train.ppo.shared_parameters: 1 = no critic_mlp, value = value(actor_mlp(x))
                                       * (models_split.py:100-102, 226-230); 0 = separate critic.  Not with contacts. */
  /* Python-float (double) hyper-parameters: the reference multiplies them as doubles before the
   * tensor op casts to fp32 (e.g. gamma*tau, experience.py:254; Adam bias corrections). */
  double gamma, tau;                  /* experience.py:242-255 */
  double lr, beta1, beta2, adam_eps;  /* torch.optim.Adam (frozen_ppo.py:192-194) */
  float e_clip, critic_coef, entropy_coef, bounds_loss_coef; /* frozen_ppo.py:543-564 */
  float grad_norm;                    /* clip_grad_norm_ max norm; <=0: no clipping (:608-609) */
  float rms_eps;                      /* running_mean_std.py:24 (1e-5) */
  /* ground-truth contacts (task.env.compute_contact_gt; models_split.py:41-55, 81-88, 172-177); all zero = off.
   * contact_points = num_points P, contact_emb = contact_mlp.units[-1] (<= 32), only_contact = train.ppo.only_contact
   * (the trunk then sees [obs | contact embedding] and env_mlp is not trained; needs contact_emb == priv_units[-1]). */
  int32_t contact_points, contact_emb, only_contact;
  /* KL-adaptive learning rate (rl_games AdaptiveScheduler, schedule_type standard; frozen_ppo.py:624-630, 864-877 with
   * the scheduler call of :630 live -- an opt-in beyond the reference's live code); all zero = fixed: the rate is
   * cfg.lr.  lr_schedule 1: the rate lives in st->lr_state, Adam reads it there, and after the last optimizer step of
   * every mini-epoch a one-wave kernel applies  lr = max(lr / 1.5, lr_min) if kl > 2 kl_threshold,
   * lr = min(lr * 1.5, lr_max) if kl < 0.5 kl_threshold  (in double, strict inequalities) to that mini-epoch's mean KL;
   * cfg.lr is then ignored.  The host neither reads nor writes the rate during an update. */
  int32_t lr_schedule;
  double kl_threshold, lr_min, lr_max;
} igi_teacher_cfg;

/* Time-major rollout arena, exactly what play_steps stores (frozen_ppo.py:655-683;
 * experience.py:163-185): obses (T,N,obs) priv_info (T,N,priv) rewards/values (T,N,1)
 * neglogpacs (T,N) dones (T,N) u8 actions/mus/sigmas (T,N,act); last_values (N,1). */
typedef struct igi_rollout {
  const float* obses;
  const float* priv_info;
  const float* rewards;
  const float* values;
  const float* neglogpacs;
  const uint8_t* dones;
  const float* actions;
  const float* mus;
  const float* sigmas;
  const float* last_values;
  const float* contacts;   /* (T,N,contact_points); required when the cfg enables contacts, else ignored */
} igi_rollout;

/* Trainer-owned persistent state. */
typedef struct igi_teacher_state {
  float* params;      /* flat fp32, ActorCriticSplit.state_dict() order, every
                         tensor starting on a 16-byte boundary: see igi_teacher_param_offsets */
  float* grads;       /* flat fp32 gradient of the last minibatch (pre-clip), same layout */
  float* adam_m;      /* exp_avg */
  float* adam_v;      /* exp_avg_sq */
  double* rms_obs;    /* [mean(obs_dim), var(obs_dim), count] */
  double* rms_priv;   /* [mean(priv_dim), var(priv_dim), count] */
  double* rms_value;  /* [mean, var, count] */
  const int64_t* perm;/* fixed permutation of env-major sample ids (experience.py:202) */
  /* prepared per-update data, time-major index t*N+n (written by igi_teacher_prepare): */
  float* returns_raw; /* (T,N) GAE returns before normalisation */
  float* advantages;  /* (T,N) normalised advantages */
  float* values_n;    /* (T,N) normalised old values */
  float* returns_n;   /* (T,N) normalised returns */
  float* mus_w;       /* (T,N,act) working copy, overwritten by update_mu_sigma */
  float* sigmas_w;    /* (T,N,act) */
  float* stats;       /* [E*E][IGI_STATS_PER_STEP] per-optimizer-step scalars, see below */
  void* workspace;
  size_t workspace_bytes;
  /* cfg.lr_schedule != 0 only (else ignored, may be NULL): IGI_LR_STATE_DOUBLES(mini_epochs) doubles.
   * [0] the learning rate: the caller writes it before the first update, the scheduler kernel afterwards;
   * [1] scratch of the data-parallel updates: its first 4 bytes hold, as ONE float, this rank's mini-epoch KL, summed
   *     over the ranks in place (the callback path hands it to the reducer as bucket 3);
   * [2 + 2e], [3 + 2e] the record of mini-epoch e of the last update: the KL as compared, the rate after the decision. */
  double* lr_state;
} igi_teacher_state;
#define IGI_LR_STATE_DOUBLES(mini_epochs) (2 + 2 * (mini_epochs))

/* stats row: a_loss, c_loss, b_loss, entropy, kl, grad_total_norm (pre-clip), param_norm, clip coefficient -- or, with
 * cfg.lr_schedule != 0, in the last slot the (float) learning rate the step used */
#define IGI_STATS_PER_STEP 8

/* Flat parameter vector: tensors in state_dict order (sigma, env_mlp.mlp.{0,2,..}.{weight,bias},
 * actor_mlp..., critic_mlp... (absent with cfg.shared_parameters), value.{weight,bias}, mu.{weight,bias}); each tensor starts at a
 * multiple of 4 floats (gaps are zero and stay zero).  igi_teacher_param_count = padded length;
 * igi_teacher_param_offsets fills offsets_host[i] / sizes_host[i] for tensor i and returns the
 * number of tensors (or a negative error); either array may be NULL. */
int64_t igi_teacher_param_count(const igi_teacher_cfg* cfg);
int igi_teacher_param_offsets(const igi_teacher_cfg* cfg, int64_t* offsets_host, int64_t* sizes_host,
                              int max_tensors);
size_t igi_teacher_workspace_bytes(const igi_teacher_cfg* cfg);

/* computer_return + prepare_training + value normalisation tail
 * (experience.py:242-263, frozen_ppo.py:717-725).  No transposed copies are made: sample id
 * b = n*T+t of the reference's env-major flattening addresses element t*N+n.
 * normalize_value == 0 (ppo.normalize_value False, frozen_ppo.py:719) leaves rms_value untouched
 * and copies values / returns through un-normalised. */
int igi_teacher_prepare(const igi_teacher_cfg* cfg, const igi_rollout* ro,
                        const igi_teacher_state* st, int normalize_value, igi_stream_t stream);

/* One optimizer step of the minibatch loop, split so a gradient all-reduce can sit between
 * (frozen_ppo.py:518-584 = fwd_bwd; :586-603 = caller's all-reduce on st->grads; :605-618 = apply).
 *   mb_index : which minibatch of the fixed permutation (experience.py:207-226)
 *   step_slot: row of st->stats to fill
 *   adam_t   : 1-based Adam step count;  grad_scale: 1/world_size folded into the optimizer. */
int igi_teacher_fwd_bwd(const igi_teacher_cfg* cfg, const igi_rollout* ro,
                        const igi_teacher_state* st, int mb_index, int step_slot,
                        igi_stream_t stream);
/* With cfg.lr_schedule != 0 igi_teacher_apply also runs the scheduler when step_slot is the last of a mini-epoch
 * (single rank: the mini-epoch's KL is this rank's). */
int igi_teacher_apply(const igi_teacher_cfg* cfg, const igi_teacher_state* st, int step_slot,
                      int64_t adam_t, float grad_scale, igi_stream_t stream);

/* Data-parallel variant of igi_teacher_fwd_bwd in two phases, so that the all-reduce of the large gradient
 * bucket overlaps the rest of backward (the reference reduces all gradients after backward,
 * frozen_ppo.py:586-603; BASELINE north_star asks for the overlap).  The cut follows the backward levels, so the two
 * phases launch exactly the kernels of igi_teacher_fwd_bwd plus one more call of the slab reduction:
 *   phase 0: gather, forward, losses, trunk backward down to dZ of the first trunk layer, heads.  On return (in stream
 *            order) the EARLY bucket is final -> start its all-reduce: actor layers >= 1 | critic layers >= 1, value, mu.
 *   phase 1: latent and env_mlp backward + the first trunk layer's weight gradient.  The LATE bucket is final:
 *            sigma, env_mlp, actor layer 0 | critic layer 0.
 * igi_teacher_grad_buckets writes the four ranges (offset, length in floats) of the flat gradient: [0], [1] early,
 * [2], [3] late (the critic's first layer sits between the two early ranges; a length may be 0) and returns 4.
 * With cfg.shared_parameters there is no critic block: [0] = actor layers >= 1, value, mu; [2] as above; [1], [3] empty.
 * Both phases of a step take the same (mb_index, step_slot); results equal igi_teacher_fwd_bwd bit for bit. */
int igi_teacher_fwd_bwd_phase(const igi_teacher_cfg* cfg, const igi_rollout* ro,
                              const igi_teacher_state* st, int mb_index, int step_slot, int phase,
                              igi_stream_t stream);
int igi_teacher_grad_buckets(const igi_teacher_cfg* cfg, int64_t* offsets, int64_t* lengths);

/* Whole single-GPU update: mini_epochs x n_minibatch (fwd_bwd + apply), enqueued back to back
 * with no host synchronisation (frozen_ppo.py:508-640).  adam_t0 = steps taken before.  Bit-identical to the
 * igi_teacher_fwd_bwd / igi_teacher_apply loop and to the data-parallel updates on one rank. */
int igi_teacher_update(const igi_teacher_cfg* cfg, const igi_rollout* ro,
                       const igi_teacher_state* st, int64_t adam_t0, igi_stream_t stream);
/* ---- KL early stopping (frozen_ppo.py:578-581 and :642-643 made live, with the estimator of :568-569; an opt-in
 * beyond the reference's live code -- rl_games / SB3 `target_kl`).  It rides beside the two structs above, which keep
 * their layout (ABI 6): the three entry points below take the same arguments as their namesakes plus this record, and
 * with ks == NULL or ks->kl_early_stop == 0 they ARE their namesakes.
 *   approx_kl_s = mean_b((exp(d_b) - 1) - d_b), d_b = neglogp_new_b - neglogp_old_b, per sample in fp32, summed in
 *   double (column 5 of the loss record), / mb.  Optimizer step s stops the update iff
 *   (double)(float)approx_kl_s > 1.5 * kl_threshold (strict, in double).  The statistics block of the norm kernel
 *   takes the decision ahead of the Adam launch of the same step; from then on both halves of the fused Adam + gather
 *   launch, the stand-alone gather, the update_mu_sigma write-back, the statistics rows and the learning-rate
 *   scheduler of every later mini-epoch are inert: parameters, Adam moments, first-layer copies and normaliser state are
 *   those after step s - 1 (the normalisers have ingested minibatch s, frozen_ppo.py:521-522).  Row s of st->stats holds
 *   slots 0 .. 4 (entropy and KL are appended before the reference's break), rows behind it are unspecified.  With
 *   cfg.lr_schedule != 0 the scheduler of the stopping mini-epoch runs on the mean KL of its steps 0 .. s % n_mb (:630 sits
 *   between the two breaks).  One deviation: the loss kernel of step s has written its minibatch's mus_w / sigmas_w rows
 *   before the decision falls.
 * stop_state: IGI_STOP_STATE_WORDS(mini_epochs * n_minibatch) 32-bit words, device memory.
 *   [0] int32: the stop step of the last update, -1 = it ran through (step 0 of every update resets it);
 *   [1] float: scratch of the data-parallel updates -- this rank's estimator of the step, summed over the ranks in
 *       place;  [2 + s] float: approx_kl of step s (data parallel: the rank mean, as compared).
 * igi_teacher_update_ks stops ENQUEUEING one mini-epoch behind the decision: after it has enqueued mini-epoch e + 1 it
 * waits for an event recorded behind mini-epoch e and reads word 0 through a copy stream of its own that waits for
 * that event only -- one host wait per mini-epoch, none when the switch is off.  Not capturable into a graph.
 * Data parallel (igi_teacher_update_dp_ks, igi_teacher_update_dp_rccl_ks; declared behind their namesakes): all ranks
 * take the decision from the rank-mean estimator.  Per optimizer step, between the norm kernel and the Adam tail, the
 * rank's fp32 mean goes into the scratch float, that ONE float is all-reduced (SUM) -- callback path: reduce(user, 4,
 * step), in the order of `stream`; RCCL path: on `stream`, behind the join of the step's gradient collectives -- and a
 * one-lane kernel divides by the world size in fp32 and compares: the same bits, the same stop step and the same
 * look-ahead boundary on every rank.  With cfg.lr_schedule != 0, ks->kl_threshold must equal cfg->kl_threshold. */
typedef struct igi_kl_stop {
  int32_t kl_early_stop;  /* 0 = off */
  double kl_threshold;    /* > 0 */
  int32_t* stop_state;
} igi_kl_stop;
#define IGI_STOP_STATE_WORDS(steps) (2 + (steps))
int igi_teacher_fwd_bwd_ks(const igi_teacher_cfg* cfg, const igi_rollout* ro, const igi_teacher_state* st,
                           const igi_kl_stop* ks, int mb_index, int step_slot, igi_stream_t stream);
int igi_teacher_apply_ks(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const igi_kl_stop* ks, int step_slot,
                         int64_t adam_t, float grad_scale, igi_stream_t stream);
int igi_teacher_update_ks(const igi_teacher_cfg* cfg, const igi_rollout* ro, const igi_teacher_state* st,
                          const igi_kl_stop* ks, int64_t adam_t0, igi_stream_t stream);

/* The packed configuration of the mi355ppo ops, (int[] icfg, float[] fcfg) (the layout is written once, in
 * csrc/teacher_cfg.h), decoded and validated: fills *cfg; with ks != NULL also ks->kl_early_stop / kl_threshold from the
 * early-stopping tail (zeroed when the lists carry none; stop_state stays NULL, the caller owns that tensor), with
 * ks == NULL a list carrying the tail is refused for its length.  Host only, no GPU work.  Returns the number of optimizer
 * steps the stop record covers (the argument of IGI_STOP_STATE_WORDS; 0 without a tail), or IGI_E_BADARG with the
 * specific reason in igi_last_error(). */
int64_t igi_teacher_cfg_unpack(const int64_t* icfg, int n_int, const double* fcfg, int n_float, igi_teacher_cfg* cfg,
                               igi_kl_stop* ks);

/* Latent-gradient fusion of the teacher backward (default ON; IGI_LATZ_FUSE=0 in the environment starts it off;
 * profiles/r06_latz_ab.log): the backward of env_mlp's last (8-wide) layer -- d(latent) from the first trunk layer's row dots,
 * its rank-8 weight / bias gradient and dZ of the 128-wide layer below (autograd of models_split.py:185-232 as called from
 * frozen_ppo.py:583-585) -- happens at the head of every row block of the env level's row-block kernel instead of in a launch
 * of its own (9 launches per optimizer step instead of 10, dZ of that layer never reaches HBM).  dZ is formed by the same
 * expressions (bit-identical); the latent layer's weight gradient is summed on the matrix pipe per row range instead of per 32
 * rows, so it differs in the last bits.  Reference shapes only (priv_units [256, 128, 8]); anything else keeps the separate
 * launch whatever the setting.  Returns the previous setting. */
int igi_teacher_set_latz_fuse(int on);

/* Whole DATA-PARALLEL update as ONE host call (frozen_ppo.py:508-640 with the gradient exchange of :586-603):
 * per optimizer step the library enqueues phase 0, calls reduce(user, 0, step) -- the caller starts the all-reduce
 * (SUM) of grads[grad_split : param_count) on its communication stream and returns without blocking --, enqueues
 * phase 1, calls reduce(user, 1, step) for grads[0 : grad_split), then reduce(user, 2, step) -- the caller makes
 * `stream` wait (stream-ordered, no host block) for both collectives -- and enqueues clip + Adam with grad_scale
 * (= 1 / world_size).  reduce returns 0, or non-zero to abort (returned as IGI_E_CALLBACK).  The callback is the
 * only thing that is not a kernel launch: there is no per-step host <-> library round trip besides it.
 * With cfg.lr_schedule != 0, after the last step of every mini-epoch the library writes this rank's mean KL as one
 * float at (float*)(st->lr_state + 1) and calls reduce(user, 3, step): the caller all-reduces (SUM) that ONE float in
 * place, in the order of `stream` (or makes `stream` wait for it); the scheduler kernel then divides by
 * 1 / grad_scale ranks and decides -- identically on every rank (frozen_ppo.py:625-627). */
typedef int (*igi_reduce_fn)(void* user, int bucket, int step);
int igi_teacher_update_dp(const igi_teacher_cfg* cfg, const igi_rollout* ro, const igi_teacher_state* st,
                          int64_t adam_t0, float grad_scale, igi_reduce_fn reduce, void* user, igi_stream_t stream);
int igi_teacher_update_dp_ks(const igi_teacher_cfg* cfg, const igi_rollout* ro, const igi_teacher_state* st,
                             const igi_kl_stop* ks, int64_t adam_t0, float grad_scale, igi_reduce_fn reduce, void* user,
                             igi_stream_t stream);

/* ---- RCCL communicator owned by the library (replaces dist.init_process_group("nccl") + the per-step
 * torch.cat / dist.all_reduce / copy-back of frozen_ppo.py:116-126, 586-603 and ext_adapt.py:833-851).
 * One process per GPU.  Rank 0 draws an id (igi_comm_unique_id, 128 bytes), hands it to every rank by any means
 * (the Python layer uses torch.distributed's store), and every rank calls igi_comm_create on ITS device: the object
 * holds the ncclComm_t, a communication stream and the events that fence it against the compute stream
 * (system-scope events when world > 1, device-scope on a one-rank communicator; IGI_EVENT_SYSFENCE=0 / 1 overrides).
 * A failing igi_comm_create releases everything it had built, sets *out = NULL and leaves the reason in
 * igi_comm_last_error(NULL) (per thread). */
#define IGI_COMM_ID_BYTES 128
typedef struct igi_comm* igi_comm_t;
int igi_comm_unique_id(void* id128);
int igi_comm_create(const void* id128, int rank, int world, igi_comm_t* out);
int igi_comm_destroy(igi_comm_t comm);
int igi_comm_rank(igi_comm_t comm);
int igi_comm_world(igi_comm_t comm);
/* What RCCL itself says about the communicator: ncclCommCount (the number of ranks RCCL connected -- igi_comm_world
 * returns the value the caller passed to igi_comm_create) or a negative IGI_E_* code; and RCCL's version
 * (ncclGetVersion: major * 10000 + minor * 100 + patch), no communicator needed.  A benchmark record that carries both can
 * show that an N-GPU run really exchanged gradients among N ranks (frozen_ppo.py:119-121 reads WORLD_SIZE only). */
int igi_comm_count(igi_comm_t comm);
int igi_rccl_version(void);
const char* igi_comm_last_error(igi_comm_t comm);
/* in place, SUM, enqueued on `stream` (stream-ordered; the host does not block) */
int igi_comm_all_reduce_sum_f32(igi_comm_t comm, float* buf, int64_t n, igi_stream_t stream);
/* The same reduction on the communicator's own stream, ordered behind everything enqueued on `compute_stream` so far
 * (event fence; the host does not block): work enqueued on `compute_stream` afterwards overlaps the collective -- the
 * student's early gradient bucket (decoder side, final first) under the encoders' backward; ext_adapt.py:833-851 reduces
 * everything after backward.  igi_comm_join makes `compute_stream` wait for the last such reduction.  One in flight at
 * a time per communicator. */
int igi_comm_all_reduce_async_f32(igi_comm_t comm, float* buf, int64_t n, igi_stream_t compute_stream);
int igi_comm_join(igi_comm_t comm, igi_stream_t compute_stream);
/* parameter broadcast at the start of training (frozen_ppo.py:376-381 pickles a state_dict; here: the flat vector) */
int igi_comm_broadcast(igi_comm_t comm, void* buf, int64_t bytes, int root, igi_stream_t stream);

/* Whole data-parallel update as ONE host call with the gradient exchange issued by the library: per optimizer step
 * phase 0 -> [comm stream] all-reduce of the early bucket -> phase 1 (runs meanwhile) -> all-reduce of the late bucket
 * -> clip + Adam with grad_scale = 1 / world; events only, no callback, no host synchronisation.  overlap == 0: the
 * reference's serial schedule (one all-reduce of the whole flat gradient after backward, on `stream`).
 * stats_sum: NULL, or mini_epochs * n_minibatch * IGI_STATS_PER_STEP floats receiving st->stats summed over the
 * ranks (the per-mini-epoch KL all-reduce of frozen_ppo.py:624-627 and the loss aggregation of :387-396 as one
 * collective per update).  The learning-rate broadcast of :632-637 has nothing to send: under the fixed schedule the
 * rate is constant (the scheduler call is commented out in the reference, :630); with cfg.lr_schedule != 0 every rank
 * takes the same decision from the rank-mean KL -- one float per mini-epoch all-reduced on `stream` after the step's
 * gradient collectives were joined there, so never two collectives of the communicator on two streams -- and holds
 * the same rate. */
int igi_teacher_update_dp_rccl(const igi_teacher_cfg* cfg, const igi_rollout* ro, const igi_teacher_state* st,
                               int64_t adam_t0, igi_comm_t comm, int overlap, float* stats_sum, igi_stream_t stream);
int igi_teacher_update_dp_rccl_ks(const igi_teacher_cfg* cfg, const igi_rollout* ro, const igi_teacher_state* st,
                                  const igi_kl_stop* ks, int64_t adam_t0, igi_comm_t comm, int overlap, float* stats_sum,
                                  igi_stream_t stream);

/* Inference forward used by model_act / act_inference (models_split.py:120-164; frozen_ppo.py:343-366).
 * normalize != 0: obs/priv are raw and are normalised with the CURRENT running stats (eval mode,
 * frozen_ppo.py:345-346); normalize == 0: they are used as given (ActorCriticSplit.act receives
 * already-processed inputs).  Writes mu (rows,act), value (rows,1) (normalised scale) and latent
 * (rows, priv_units[-1]).  Any output may be NULL. */
int igi_teacher_infer(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const float* obs,
                      const float* priv, int64_t rows, int normalize, float* mu, float* value,
                      float* latent, igi_stream_t stream);

/* The policy side of ONE environment step of play_steps as one call (frozen_ppo.py:343-366 model_act + :655-665 buffer
 * writes): igi_teacher_infer (normalise with the current running statistics when normalize != 0, env_mlp, trunk, heads)
 * and igi_rollout_act_store (sample with the caller's noise, neglogp, value de-normalisation with rms_value
 * ([mean, var, count], may be NULL), arena-slot writes, clamped actions) fused: 7-8 launches, bit-identical results.
 * obses_t / priv_t (raw copies into the arena slot) may be NULL; the other outputs are required:
 * actions_t / mus_t / sigmas_t / actions_clamped (rows, act), neglogp_t / values_t / values_out (rows). */
int igi_rollout_policy_step(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const float* obs,
                            const float* priv, int64_t rows, int normalize, const float* noise,
                            const double* rms_value, float* obses_t, float* priv_t, float* actions_t,
                            float* neglogp_t, float* values_t, float* mus_t, float* sigmas_t, float* actions_clamped,
                            float* values_out, igi_stream_t stream);

/* The two calls above for a teacher with ground-truth contacts: contacts (rows, contact_points), raw (not normalised,
 * models_split.py:174).  latent of igi_teacher_infer_contacts is (rows, priv_units[-1] + contact_emb), or
 * (rows, contact_emb) with only_contact.  The calls without contacts refuse such a cfg.  contacts_t (may be NULL):
 * slot t of the (T, N, contact_points) arena, written with the raw contacts like obses_t / priv_t. */
int igi_teacher_infer_contacts(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const float* obs,
                               const float* priv, const float* contacts, int64_t rows, int normalize, float* mu,
                               float* value, float* latent, igi_stream_t stream);
int igi_rollout_policy_step_contacts(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const float* obs,
                                     const float* priv, const float* contacts, int64_t rows, int normalize,
                                     const float* noise, const double* rms_value, float* obses_t, float* priv_t,
                                     float* contacts_t, float* actions_t, float* neglogp_t, float* values_t, float* mus_t, float* sigmas_t,
                                     float* actions_clamped, float* values_out, igi_stream_t stream);

/* The contact encoder alone (ContactAE.forward_enc, models_split.py:44-51), the kernels of the teacher's contact mode.
 * Row i of the batch is row i of contacts (rows, P).  params = [W1 (32,P) | b1 (32) | W2 (E,32) | b2 (E)] packed.
 * forward: emb (rows, E), hidden (rows, 32) = relu(C W1^T + b1).  backward: from d(pre-tanh) dz (rows, E) and that
 * hidden, grads (packed like params) = the sums over the rows; workspace of
 * igi_contact_encoder_workspace_bytes(rows, P, E) bytes. */
int igi_contact_encoder_forward(const float* contacts, int64_t rows, int P, int E, const float* params, float* emb,
                                float* hidden, igi_stream_t stream);
size_t igi_contact_encoder_workspace_bytes(int64_t rows, int P, int E);
int igi_contact_encoder_backward(const float* contacts, int64_t rows, int P, int E, const float* params,
                                 const float* hidden, const float* dz, float* grads, void* workspace,
                                 size_t workspace_bytes, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rollout-side bookkeeping of PPO.play_steps, two launches per environment step.
 * igi_rollout_act_store (frozen_ppo.py:343-366, 655-665): from the policy outputs of N environments (mu (N,act),
 * value_n (N,1) on the normalised scale, logstd (act), noise (N,act) ~ N(0,1) supplied by the caller's generator):
 * sigma = exp(logstd), action = mu + sigma*noise, neglogp = -Normal(mu,sigma).log_prob(action).sum(-1), value =
 * sqrt(var+eps)*clamp(value_n,+-5)+mean when rms_value ([mean,var,count]) is given, else value_n.  Writes slot t of
 * the time-major arena -- the *_t pointers address that slot: obses_t (N,obs) priv_t (N,priv) actions_t / mus_t /
 * sigmas_t (N,act) neglogp_t (N) values_t (N) -- plus actions_clamped (N,act) = clamp(action,+-1) for env.step and
 * values_out (N).
 * igi_rollout_env_store (frozen_ppo.py:671-700): dones_t = dones; rewards_t = 0.01 r + gamma*value*time_out when
 * bootstrap != 0 and time_outs != NULL, else r; cur_rewards / cur_lengths / cur_success (N) accumulate r / 1 /
 * successes and are zeroed where done; meter[0..3] += {sum reward, sum length, sum success, count} of the episodes
 * that ended in this step (caller zeroes meter).
 * ---------------------------------------------------------------------------------------- */
int igi_rollout_act_store(int64_t n_envs, int obs_dim, int priv_dim, int act_dim, const float* obs,
                          const float* priv, const float* mu, const float* value_n, const float* logstd,
                          const float* noise, const double* rms_value, float eps, float* obses_t, float* priv_t,
                          float* actions_t, float* neglogp_t, float* values_t, float* mus_t, float* sigmas_t,
                          float* actions_clamped, float* values_out, igi_stream_t stream);
int igi_rollout_env_store(int64_t n_envs, const float* rewards, const uint8_t* dones, const float* values,
                          const uint8_t* time_outs, const float* successes, float gamma, int bootstrap,
                          float* rewards_t, uint8_t* dones_t, float* cur_rewards, float* cur_lengths,
                          float* cur_success, float* meter, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Student distillation loss (ext_adapt.py:812-819): loss[0] = sum over rows and action dims of
 * weights[q] * (clamp(mu,+-1) - clamp(teacher,+-1))^2 (a SUM; the reference's trailing .mean() acts on a scalar), and,
 * when dmu != NULL, dmu = d loss / d mu = 2 weights[q] (clamp(mu) - clamp(teacher)) where -1 <= mu <= 1, else 0.
 * Fixed-order fp64 partial sums.  workspace >= igi_bc_loss_workspace_bytes().
 * ---------------------------------------------------------------------------------------- */
size_t igi_bc_loss_workspace_bytes(void);
int igi_bc_loss(const float* mu, const float* teacher_actions, const float* weights, int64_t rows, int act_dim,
                float* loss, float* dmu, void* workspace, size_t workspace_bytes, igi_stream_t stream);

/* The latent student's loss (offline_train.train.latent_loss; ext_adapt.py:827 with the latent term live) in ONE launch:
 * loss_action[0] as igi_bc_loss's loss, loss_latent[0] = mean((latent - latent_gt)^2) over (rows, latent_dim),
 * dmu (rows, act_dim) = action_scale * d loss_action / d mu, dlatent (rows, latent_dim) = latent_scale * 2 (latent -
 * latent_gt) / (rows * latent_dim): the gradients of action_scale * loss_action + latent_scale * loss_latent.  Every
 * pointer is required.  Fixed-order fp64 sums. */
int igi_distill_loss(const float* mu, const float* teacher_actions, const float* weights, int64_t rows, int act_dim,
                     const float* latent, const float* latent_gt, int latent_dim, float action_scale, float latent_scale,
                     float* loss_action, float* loss_latent, float* dmu, float* dlatent, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The frozen actor on [obs | student latent] (ActorCriticSplit.act_inference / act_with_grad with a `latent` entry:
 * ext_adapt.py:684-690, 799-806): mu (rows, act) = mu head(actor_mlp(cat(obs_n, latent))), no value, no critic.
 * obs_n (rows, obs_dim) normalised, latent (rows, latent_dim) with latent_dim = the teacher's own extrinsic width
 * (priv_units[-1], plus the contact embedding of a contact teacher), IGI_E_BADARG otherwise.  With the reference's layer
 * sizes (units 512 / 256 / 128, obs_dim + latent_dim <= 32, act <= 7) the forward is k_pad_w1 + one k_actor_latent launch
 * per chunk of minibatch rows; every other shape runs the actor's layers one launch each.  Uses state.workspace.
 * hsave (may be NULL): (rows, igi_actor_latent_saved_width(cfg)) = the post-tanh activations of the actor's layers side
 * by side, each layer's width rounded up to 4 -- the caller's buffer, handed back to igi_actor_latent_backward, which
 * writes dlatent (rows, latent_dim) = d/d latent of a loss with gradient dmu (rows, act).  No weight gradient.
 * ---------------------------------------------------------------------------------------- */
int igi_actor_latent_saved_width(const igi_teacher_cfg* cfg);
/* latent_dim above: the width of the latent igi_teacher_infer[_contacts] writes and of dlatent; 0 for a cfg the library refuses */
int igi_teacher_latent_width(const igi_teacher_cfg* cfg);
int igi_actor_latent_forward(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const float* obs_n,
                             const float* latent, int latent_dim, int64_t rows, float* mu, float* hsave,
                             igi_stream_t stream);
int igi_actor_latent_backward(const igi_teacher_cfg* cfg, const igi_teacher_state* st, const float* hsave,
                              const float* dmu, int64_t rows, float* dlatent, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * clip_grad_norm_ + torch.optim.Adam step on one flat fp32 vector (frozen_ppo.py:608-610;
 * ext_adapt.py:853-855): grads are scaled by grad_scale (1/world after an all-reduce SUM), clipped to
 * global L2 norm max_norm (<= 0: no clipping) and applied with Adam's single-tensor update rule
 * (bias corrections from the 1-based step t).  stats_out (8 floats, may be NULL) receives
 * [.., .., .., .., .., total_norm, param_norm, clip_coef].  workspace: igi_clip_adam_workspace_bytes().
 * ---------------------------------------------------------------------------------------- */
size_t igi_clip_adam_workspace_bytes(void);
int igi_clip_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float max_norm, double lr, double beta1, double beta2, double eps, int64_t t,
                  float grad_scale, void* workspace, size_t workspace_bytes, float* stats_out,
                  igi_stream_t stream);

/* Same with decoupled weight decay = torch.optim.AdamW's single-tensor rule: param *= 1 - lr*weight_decay
 * before the Adam update (offline supervised student: runner.py:481, AdamW(lr, weight_decay=1e-6)). */
int igi_clip_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                   int64_t t, float grad_scale, void* workspace, size_t workspace_bytes, float* stats_out,
                   igi_stream_t stream);
/* As igi_clip_adamw plus torch.optim.Adam's COUPLED weight decay (ext_adapt.py:1139, phase-3 optimizer
 * Adam(lr=1e-3, weight_decay=1e-6)): after clipping, grad += l2 * param. */
int igi_clip_adam_l2(float* params, const float* grads, float* m, float* v, int64_t n, float max_norm, double lr,
                     double beta1, double beta2, double eps, double weight_decay, double l2, int64_t t,
                     float grad_scale, void* workspace, size_t workspace_bytes, float* stats_out,
                     igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One backward LEVEL of a Linear + Tanh stack as ONE persistent row-block kernel (csrc/rowblock.h): for the layer
 * Z = X W^T + b whose input X is the tanh output of the layer below,
 *     dx = (dz . weight) * (1 - x^2)      [nets][rows][in]     data gradient into the layer below, times tanh'
 *     dweight_partials, dbias_partials    [parts][nets][out][in] / [parts][nets][out]: fixed-order partial sums over
 *                                         row ranges; the caller adds the `parts` partials (igi_level_backward_parts)
 * Replaces autograd through nn.Linear + nn.Tanh (algo/models/models_split.py:27-38, reached from loss.backward(),
 * algo/ppo/frozen_ppo.py:583-585) for the 128-wide layers of the teacher: trunk layer 3 (both nets) and env_mlp layer 2.
 * Shapes: out == 128, in a multiple of 64 (<= 1024), rows a multiple of 64 (>= 256), nets 1 or 2; dense rows
 * (ld = width), 16-byte aligned pointers.  Other shapes: IGI_E_UNSUPPORTED (igi_gemm_f32 covers them).
 * dx is bit-identical to igi_gemm_f32(epilogue 2) on the same operands.
 * ---------------------------------------------------------------------------------------- */
int igi_level_backward_parts(int64_t rows, int in_features, int nets);   /* 0 when the shape is not supported */
int igi_level_backward(const float* dz, const float* weight, const float* x, float* dx, float* dweight_partials,
                       float* dbias_partials, int64_t rows, int in_features, int out_features, int nets,
                       igi_stream_t stream);
/* The same level (nets == 1) with the weight / bias gradient of the layer BELOW computed from the finished data-gradient
 * tiles instead of dx being written (csrc/rowblock.h, LOWX; the teacher's env_mlp backward, models_split.py:27-38):
 *     below_dweight_partials [parts][in][64] : sums over row ranges of dx^T . x_below,   x_below [rows][64] = the input
 *     below_dbias_partials   [parts][in]     : sums over row ranges of dx                 rows of the layer below
 * dx = (dz . weight) * (1 - x^2) is consumed element by element as the left operand of that product and never stored. */
int igi_level_backward_below(const float* dz, const float* weight, const float* x, const float* x_below,
                             float* dweight_partials, float* dbias_partials, float* below_dweight_partials,
                             float* below_dbias_partials, int64_t rows, int in_features, int out_features,
                             igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * TEST ENTRY: the grouped weight-gradient launcher (csrc/gemm_dma.h, gemm_wgrad_group) on a list of the caller's
 * choosing.  No product code calls it; it exists so that the launcher -- one grid for up to six (fp32) or four plus
 * four (bf16-input mode) problems, split-K slabs, bias sums from the tiles, batched nets, a launch of its own for any
 * problem the grid cannot take -- can be tested without a whole teacher step around it (tests/test_gpu_wgrad_group.py).
 * `count` (1..8) problems, each built as linear_backward and the teacher's backward build theirs:
 *     dweight[split][batch][out][in] = sum over the split's rows r of dz[batch][r][out]^T . x[batch][r][in]
 *     dbias  [split][batch][out]     = sum over the split's rows r of dz[batch][r][out]              (dbias may be NULL)
 * Split s covers rows [s * chunk, min(rows, (s + 1) * chunk)) with chunk = ceil(rows / splitk) rounded up to a
 * multiple of 32; the caller adds the splitk slabs.  Both outputs are dense.  Under igi_gemm_set_bf16_inputs(1) the
 * eligible problems with in_features > 64 that fit the four-entry table run with bf16-rounded operands; the bias sums
 * are fp32 sums of the un-rounded dz in either mode.  The list is handed to the launcher as it is: no tile logic here.
 * IGI_E_BADARG: count outside 1..8, a null problems / dz / x / dweight pointer, a non-positive extent, a leading
 * dimension below the row width.
 * ---------------------------------------------------------------------------------------- */
typedef struct igi_wgrad_problem {
  const float* dz;          /* [nbatch][rows][lddz], batch stride dz_batch_stride floats */
  const float* x;           /* [nbatch][rows][ldx],  batch stride x_batch_stride floats */
  float* dweight;           /* [splitk][nbatch][out_features][in_features] */
  float* dbias;             /* [splitk][nbatch][out_features], or NULL */
  int64_t dz_batch_stride, x_batch_stride;
  int32_t lddz, ldx, out_features, in_features, rows, nbatch, splitk;
} igi_wgrad_problem;
int igi_gemm_wgrad_group(const igi_wgrad_problem* problems, int count, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * nn.Linear with a fused activation, forward and backward, for the student's small MLPs: lin encoder
 * Linear(15,64)-ReLU-Linear(64,32) (tact.py:337-339), point-cloud compress (tact.py:367-369), MLPDecoder /
 * MultiLayerDecoder output stack (tact.py:137-158, 197-212), action head Linear(32,6)+Tanh (tact.py:407-410)
 * and the offline supervised loop built on them (runner.py:194-304).
 *   forward : y[rows][out] = act(x[rows][in] . weight[out][in]^T + bias)     activation: 0 none, 1 tanh, 2 relu
 *   backward: dy is the gradient w.r.t. y; dz = dy * act'(y); dx = dz . weight (dx may be NULL);
 *             dweight = dz^T x (may be NULL with dbias NULL: frozen layer, data gradient only); dbias = column sums
 *             of dz (may be NULL).  Sums over rows are split and
 *             added in a fixed order (deterministic).  bias may be NULL only when activation == 0.
 * ld* are row strides in floats.  workspace: igi_linear_workspace_bytes(rows, in, out).
 * ---------------------------------------------------------------------------------------- */
size_t igi_linear_workspace_bytes(int64_t rows, int in_features, int out_features);
int igi_linear_forward(const float* x, int ldx, const float* weight, const float* bias, float* y, int ldy,
                       int64_t rows, int in_features, int out_features, int activation, igi_stream_t stream);
int igi_linear_backward(const float* x, int ldx, const float* weight, const float* y, int ldy, const float* dy,
                        int lddy, float* dx, int lddx, float* dweight, float* dbias, int64_t rows,
                        int in_features, int out_features, int activation, void* workspace,
                        size_t workspace_bytes, igi_stream_t stream);

/* Backward of a CHAIN of such layers (an nn.Sequential of Linear + activation: tact.py:137-158, 196-212, 337-339, 367-369,
 * 407-410 under loss.backward()) as one call: dims[0 .. n_layers] are the widths (layer l: dims[l] -> dims[l + 1]),
 * acts[l] its activation, weight[l] its (out, in) matrix, y[l] its saved OUTPUT [rows][dims[l + 1]] (dense rows),
 * x the chain's input, dy the gradient w.r.t. the chain's output.  Per layer ONE grid computes the weight gradient and
 * the data gradient into the layer below, whose epilogue applies that layer's act'; every layer's split-row partials are
 * summed by one launch at the end.  Results are bit-identical to n_layers calls of igi_linear_backward.
 *   dx      : [rows][dims[0]] or NULL
 *   grads   : ONE flat buffer of igi_mlp_grad_floats() floats; dweight of layer l at w_offsets[l], dbias at b_offsets[l]
 *             (multiples of four floats)
 *   need_w  : NULL, or per layer 0 = frozen (its gradient range is left untouched) */
#define IGI_MLP_MAX_LAYERS 8
/* The same chain FORWARD as one launch (csrc/mlp_fwd.h; tact.py:137-212, 337-339, 367-369, 407-410 under forward()):
 * a workgroup carries 32 rows through every layer, hidden activations stay in LDS, y[l] = the layer outputs
 * [rows][dims[l + 1]] (row pitch ldy[l], NULL = dense) are each written once -- the tensors igi_mlp_backward reads.
 * bias[l] may be NULL only where acts[l] == 0.  Bit-identical to n_layers calls of igi_linear_forward.  Layers wider
 * than 256 outputs (and the bf16-input mode): IGI_E_UNSUPPORTED, run the layers one by one. */
int igi_mlp_forward(const float* x, int ldx, int64_t rows, int n_layers, const int32_t* dims, const int32_t* acts,
                    const float* const* weight, const float* const* bias, float* const* y, const int32_t* ldy,
                    igi_stream_t stream);
int64_t igi_mlp_grad_floats(int n_layers, const int32_t* dims, int64_t* w_offsets, int64_t* b_offsets);
size_t igi_mlp_workspace_bytes(int64_t rows, int n_layers, const int32_t* dims);
int igi_mlp_backward(const float* x, int ldx, int64_t rows, int n_layers, const int32_t* dims, const int32_t* acts,
                     const float* const* weight, const float* const* y, const float* dy, float* dx, float* grads,
                     const int32_t* need_w, void* workspace, size_t workspace_bytes, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Depth / segmentation image encoder: DepthOnlyFCBackbone54x96 (algo/models/transformer/tact.py:81-113),
 * forward and backward.  x is (batch, 1, 54, 96) fp32; y is (batch, latent_dim) BEFORE the optional output
 * activation (identity in the reference's use, tact.py:305, 323).  params / grads: flat vector in state_dict order
 * (image_compression.0.weight [32,1,5,5], .0.bias, .3.weight [64,32,3,3], .3.bias, .6.weight [128,64768], .6.bias,
 * .8.weight [latent,128], .8.bias).  backward needs the workspace forward filled and the same x; the input gets
 * no gradient (it is an observation).  batch must be a multiple of 32, latent_dim of 4.
 * ---------------------------------------------------------------------------------------- */
typedef struct igi_depth_cfg {
  int32_t batch, latent_dim;
} igi_depth_cfg;
int64_t igi_depth_param_count(const igi_depth_cfg* cfg);
size_t igi_depth_workspace_bytes(const igi_depth_cfg* cfg);
int igi_depth_forward(const igi_depth_cfg* cfg, const float* x, const float* params, float* y, void* workspace,
                      size_t workspace_bytes, igi_stream_t stream);
int igi_depth_backward(const igi_depth_cfg* cfg, const float* x, const float* dy, const float* params, float* grads,
                       void* workspace, size_t workspace_bytes, igi_stream_t stream);
/* Where igi_depth_forward leaves its activations in the workspace (diagnostics / parity tests): byte offsets[3] and rows[3]
 * of a1 = ELU(max-pool(conv1)) (batch * 25 * 46 rows of 32, channels-last), a2 = ELU(conv2) (batch * 23 * 44 rows of 64,
 * channels-last: a row of the big Linear's input is an image's 1012 rows) and h3 = ELU(Linear 64768 -> 128) (batch rows of
 * 128), all fp32.  The pool's arg-max bytes (uint8, one per element of a1: 2 * dy + dx inside the 2 x 2 window) start
 * right behind a1, at offsets[0] + 4 * 32 * rows[0].  Returns 0, or an error for a configuration the backbone rejects. */
int igi_depth_activation_layout(const igi_depth_cfg* cfg, int64_t offsets[3], int64_t rows[3]);

/* ------------------------------------------------------------------------------------------
 * Token decoder of the student: `layers` x nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward ff,
 * activation "gelu", batch_first, norm_first) over `seq` <= 32 tokens per sample
 * (algo/models/transformer/tact.py:137-158: MultiLayerDecoder.sa_decoder), forward and backward.
 * Supported: d_model in {32, 64, 128}; nhead with d_model / nhead in {16, 32, 64}; seq <= 32; ff a multiple of 4;
 * layers <= 8; batch * seq <= 2^26.  Anything else: IGI_E_UNSUPPORTED (there is no fallback).
 *   (32, 2), the reference's stock config: seq <= 8 attention in registers, 16 lanes per (sample, head); 9 .. 32 one
 *     32 x 32 MFMA tile per (sample, head); one-launch forward / backward kernels where ff = 128 and the shape allows.
 *   every other (d_model, nhead): one launch per operation, LayerNorm with a wave per row, attention on the MFMA tile
 *     at every seq (heads of 64 in two column passes).
 * x, y, dy, dx: (batch, seq, d_model) fp32.  params / grads: layers x igi_token_param_count()/layers floats, each layer
 * in nn.TransformerEncoderLayer's parameter order (in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias,
 * linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.weight, norm1.bias, norm2.weight, norm2.bias).
 * training != 0 applies the layer's four dropouts (attention probabilities, both residual branches, after the
 * activation) with probability `dropout`; masks are a counter-based function of `seed` (pass the same seed and the
 * same workspace to backward; nothing else is retained between the two calls).
 * ---------------------------------------------------------------------------------------- */
typedef struct igi_token_cfg {
  int32_t batch, seq, d_model, nhead, ff, layers;
  float dropout;
  int32_t training;
} igi_token_cfg;
int64_t igi_token_param_count(const igi_token_cfg* cfg);
size_t igi_token_workspace_bytes(const igi_token_cfg* cfg);
int igi_token_forward(const igi_token_cfg* cfg, const float* x, const float* params, float* y, void* workspace,
                      size_t workspace_bytes, uint64_t seed, igi_stream_t stream);
int igi_token_backward(const igi_token_cfg* cfg, const float* dy, const float* params, float* dx, float* grads,
                       void* workspace, size_t workspace_bytes, uint64_t seed, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AllSight tactile encoder: CNNWithSpatialSoftArgmax (algo/models/transformer/tactile_cnn.py:7-79),
 * forward and backward.  x is (batch, 3, height, width) fp32 NCHW as the reference feeds it
 * (3 fingers' gray images stacked as channels; runner.py:397-400, tact.py:431-432); y is
 * (batch, latent_dim).  params / grads are flat fp32 in the module's state_dict order:
 * cnn.0.weight (32,3,8,8) cnn.0.bias cnn.2.weight (64,32,4,4) cnn.2.bias cnn.4.weight (64,64,3,3)
 * cnn.4.bias cnn.7.weight (latent,128) cnn.7.bias.  batch must be a multiple of 32.
 * igi_tactile_backward must follow igi_tactile_forward on the same workspace (saved activations)
 * and under the same igi_conv_set_bf16_inputs setting;
 * it overwrites `grads` with d(loss)/d(params) given dy = d(loss)/d(y).
 * ---------------------------------------------------------------------------------------- */
typedef struct igi_tactile_cfg {
  int32_t batch, height, width, latent_dim;
} igi_tactile_cfg;
int64_t igi_tactile_param_count(const igi_tactile_cfg* cfg);
size_t igi_tactile_workspace_bytes(const igi_tactile_cfg* cfg);
int igi_tactile_forward(const igi_tactile_cfg* cfg, const float* x, const float* params, float* y,
                        void* workspace, size_t workspace_bytes, igi_stream_t stream);
int igi_tactile_backward(const igi_tactile_cfg* cfg, const float* dy, const float* params, float* grads,
                         void* workspace, size_t workspace_bytes, igi_stream_t stream);
/* Where igi_tactile_forward leaves the three activated feature maps in its workspace (diagnostics / parity tests: which
 * side of a ReLU a pre-activation fell on): byte offsets[3] and rows[3] = batch * H_out * W_out of conv 1..3; each map is
 * channels-last (rows, 32 | 64 | 64) fp32.  Returns 0, or an error for a configuration the encoder rejects. */
int igi_tactile_activation_layout(const igi_tactile_cfg* cfg, int64_t offsets[3], int64_t rows[3]);

/* Standalone SpatialSoftArgmax.forward (algo/models/transformer/tactile_cnn.py:47-58) and its gradient, for callers
 * that use the module outside CNNWithSpatialSoftArgmax: x is (rows = B*C, h*w) contiguous (an NCHW tensor),
 * out (rows, 2) = (E[x], E[y]) with the reference's coordinate quirk (flat index k -> grid_w[k / h], grid_h[k % h]),
 * stat (rows, 2) = (row max, sum of exp) kept for the backward.  normalize != 0: linspace(-1, 1) grids, else arange. */
int igi_spatial_softargmax_forward(const float* x, int64_t rows, int h, int w, int normalize, float* out,
                                   float* stat, igi_stream_t stream);
int igi_spatial_softargmax_backward(const float* x, const float* out, const float* stat, const float* dout,
                                    int64_t rows, int h, int w, int normalize, float* dx, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmented point-cloud encoder: PointNet (algo/models/transformer/pointnets.py:12-42), forward
 * (+ argmax over the point axis) and backward.  x (batch, npoints, 3), consecutive clouds x_pitch floats apart (0 = dense;
 * > 3 npoints: a slice of a wider cloud tensor read in place, tact.py:542-566); dy (batch, 256) with rows dy_pitch floats
 * apart (0 = dense: a slice of the gradient of the concatenated encodings); y (batch, 256); argmax
 * (batch, 256) int32 point index of each column's maximum (may be NULL in forward when no backward
 * follows).  params / grads flat fp32 in state_dict order: local_mlp.0.weight (64,3),
 * local_mlp.0.bias (64), local_mlp.2.weight (256,64), local_mlp.2.bias (256) = 16896 floats.
 * Backward overwrites `grads`; workspace: igi_pointnet_workspace_bytes(batch).  1 <= npoints <= 8192 (the reference's
 * clouds hold 400 points per object; more returns IGI_E_UNSUPPORTED).  Ties between points: the first maximum in point
 * order, as torch.max.  erf-GELU: x * Phi(x) with |Phi error| <= 7.3e-8 (csrc/pointnet.h).
 * ---------------------------------------------------------------------------------------- */
#define IGI_POINTNET_PARAMS 16896
size_t igi_pointnet_workspace_bytes(int64_t batch);
int igi_pointnet_forward(const float* x, int64_t x_pitch, int64_t batch, int npoints, const float* params, float* y,
                         int32_t* argmax, igi_stream_t stream);
int igi_pointnet_backward(const float* x, int64_t x_pitch, int64_t batch, int npoints, const float* params, const float* dy,
                          int64_t dy_pitch, const int32_t* argmax, float* grads, void* workspace, size_t workspace_bytes,
                          igi_stream_t stream);
/* Several objects of ONE cloud tensor in one launch (tact.py:542-566: the plug, socket, goal ... PointNets each encode their
 * own slice of obs_pcl; here: one forward and one backward launch per step instead of one per object, and the encodings land
 * concatenated, which is what compress_pcl_enc reads, tact.py:568-571).  1 <= nobj <= 4; object i = points
 * x_off[i] / 3 ... of every cloud (x_off in floats from the cloud's first float), npoints[i] of them, parameters params[i]
 * (host array of device pointers, 16896 floats each).  y and argmax are (batch, nobj * 256): object i in columns 256 i ...;
 * dy rows dy_pitch floats apart (0 = dense nobj * 256); grads (nobj, 16896); workspace:
 * igi_pointnet_workspace_bytes_multi(batch, nobj).  Same arithmetic per object as the single-object entries (bit-identical
 * outputs; the weight-gradient partials are summed over another number of workgroups). */
size_t igi_pointnet_workspace_bytes_multi(int64_t batch, int nobj);
int igi_pointnet_forward_multi(int nobj, const float* x, int64_t x_pitch, int64_t batch, const int32_t* x_off,
                               const int32_t* npoints, const float* const* params, float* y, int32_t* argmax,
                               igi_stream_t stream);
int igi_pointnet_backward_multi(int nobj, const float* x, int64_t x_pitch, int64_t batch, const int32_t* x_off,
                                const int32_t* npoints, const float* const* params, const float* dy, int64_t dy_pitch,
                                const int32_t* argmax, float* grads, void* workspace, size_t workspace_bytes,
                                igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The student step's data movement between the blocks above (csrc/glue.h) -- pure copies, bit-exact:
 *   igi_gather_rows : dst[k][r][:] = src[k][rows[r]][:] for n <= 8 arenas of width[k] floats per row in ONE launch -- the
 *                     minibatch gather of StudentBuffer.__getitem__ (experience.py:117-139 gathers every key by itself).
 *                     A row number outside [0, rows_total) yields a NaN row.
 *   igi_cat_cols    : cat[b] = [part[0][b] | part[1][b] | ...] (+ add, one row of sum(width) floats added to every row,
 *                     or NULL): torch.cat of the encoders' tokens plus the positional encoding (tact.py:567-571, 126-135)
 *                     and of the point-cloud encodings (tact.py:566).
 *   igi_split_cols  : the reverse (the backward of the concatenation): every part dense, one launch.
 * ---------------------------------------------------------------------------------------- */
#define IGI_GLUE_MAX 8
int igi_gather_rows(int n, const float* const* src, const int64_t* width, float* const* dst, const int64_t* rows,
                    int64_t nrows, int64_t rows_total, igi_stream_t stream);
int igi_cat_cols(int n, const float* const* part, const int64_t* width, float* cat, const float* add, int64_t rows,
                 igi_stream_t stream);
int igi_split_cols(int n, float* const* part, const int64_t* width, const float* cat, int64_t rows, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-time augmentation of the offline student's camera pair (csrc/augment.h), ONE launch from the resident arenas to
 * the two batch tensors (SyncTransform of algo/models/transformer/utils.py:85-128 over a minibatch):
 *   img, seg  : fp32 [n][t][hs][ws] depth frames and segmentation masks
 *   rows      : [b] sample numbers; one outside [0, n) reads as a frame of zeros (never outside the arena)
 *   offsets   : [b][2] (top, left) of the crop window, shared by a sample's t frames and by both tensors; any value is
 *               allowed, a read outside the stored frame gives 0
 *   angles    : [b][2] radians, column 0 rotates the depth frames, column 1 the masks, about the centre of the cropped
 *               window: nearest resampling (round half to even), zero fill outside the WINDOW; angle 0 is a plain copy
 *   keep      : uint8 [b*t][out_h / patch][out_w / patch] or NULL; 0 zeroes that patch of the depth frame only; rows and
 *               columns past the last whole patch are untouched
 *   noise_std : > 0 adds noise_std * z to both outputs, z = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((h1 >> 8) + 1/2) 2^-24,
 *               u2 = (h2 >> 8) 2^-24, h1 / h2 = the token encoder's counter hash of (seed, 2 p / 2 p + 1, e): p = 0 depth,
 *               1 mask, e = the element's linear index in its output tensor.  A pure function: same arguments, same bits
 *   out_img, out_seg : fp32 [b][t][out_h][out_w], out_h <= hs, out_w <= ws
 * ---------------------------------------------------------------------------------------- */
int igi_image_pair_augment(const float* img, const float* seg, int64_t n, int t, int hs, int ws, const int64_t* rows,
                           int64_t b, const int32_t* offsets, const float* angles, const uint8_t* keep, int out_h,
                           int out_w, int patch, float noise_std, uint64_t seed, float* out_img, float* out_seg,
                           igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-time augmentation of the offline student's tactile images (csrc/tactile_augment.h), ONE launch from the resident
 * arena to the batch tensor (_Crop + _TrainAugment + GaussianNoise + Masking of algo/models/transformer/utils.py over a
 * minibatch).  An image is one (sample, t, finger) plane and has its own parameters:
 *   arena     : fp32 [n][planes][hs][ws], planes = t * fingers, one channel
 *   rows      : [b] sample numbers; one outside [0, n) reads as frames of zeros (never outside the arena)
 *   params    : int32 [b*planes][IGI_TACTILE_AUG_WORDS]: top, left of the crop window (any value; a read outside the stored
 *               frame gives 0), the jitter flag, then the fp32 bit patterns of brightness b, contrast c and the rotation
 *               angle in radians.  Flag != 0: x = clamp(x b, 0, 1), m = the image's mean (fixed summation order),
 *               x = clamp((x - m) c + m, 0, 1); flag 0: the window passes bit for bit.  The rotation is the one of
 *               igi_image_pair_augment (nearest, round half to even, zero fill outside the window; angle 0 copies) and
 *               acts on the jittered window
 *   keep      : uint8 [b*planes][out_h / patch][out_w / patch] or NULL; 0 zeroes that patch; rows and columns past the last
 *               whole patch are untouched
 *   noise_std : > 0 adds noise_std * z, z the Box-Muller sample of igi_image_pair_augment on plane p = 2 (hash sites 4 and
 *               5), e = the element's linear index in out.  A pure function: same arguments, same bits
 *   out       : fp32 [b][planes][out_h][out_w], out_h <= hs, out_w <= ws; out_h * out_w above 8192: IGI_E_UNSUPPORTED
 * ---------------------------------------------------------------------------------------- */
#define IGI_TACTILE_AUG_WORDS 6
int igi_tactile_augment(const float* arena, int64_t n, int planes, int hs, int ws, const int64_t* rows, int64_t b,
                        const int32_t* params, const uint8_t* keep, int out_h, int out_w, int patch, float noise_std,
                        uint64_t seed, float* out, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same chain for the ONLINE student's distillation step (csrc/tactile_augment_seeded.h), ONE launch from the rollout
 * storage's time-major arena to the minibatch tensor, with nothing drawn on the host but `seed`:
 *   arena     : fp32 [n][planes][hs][ws], n = horizon * envs flat rows, planes = history * fingers; never written
 *   rows      : [b] flat rows (the ones igi_gather_rows takes); one outside [0, n) reads as frames of zeros
 *   the window is the top-left out_h x out_w of the stored frame.  Per image (image = row-in-batch * planes + plane): the
 *   jitter flag (probability 0.3), brightness and contrast in 1 +- 0.1, the rotate flag (0.5), the angle in +- 3 degrees and,
 *   with masking_prob > 0, the keep value of every out_h / patch x out_w / patch patch (kept with probability
 *   1 - masking_prob) are the counter hash of (seed, site, element) at the sites tabled in csrc/tactile_augment_seeded.h,
 *   every event an integer comparison.  An image with both flags off passes bit for bit
 *   noise_std : as igi_tactile_augment, from the same seed
 *   out       : fp32 [b][planes][out_h][out_w], not the arena; out_h * out_w above 8192: IGI_E_UNSUPPORTED
 *   draws     : int32 [b*planes][IGI_TACTILE_AUG_WORDS] or NULL: 0, 0, the jitter flag, the fp32 bit patterns of b, c, angle
 *               the kernel used.  masking_prob outside [0, 1], or > 0 with patch < 1: IGI_E_BADARG.  Same arguments, same bits
 * ---------------------------------------------------------------------------------------- */
int igi_tactile_augment_seeded(const float* arena, int64_t n, int planes, int hs, int ws, const int64_t* rows, int64_t b,
                               int out_h, int out_w, int patch, float noise_std, double masking_prob, uint64_t seed,
                               float* out, int32_t* draws, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The camera pair for the ONLINE student's distillation step (csrc/augment_seeded.h), ONE launch from the rollout storage's
 * two time-major arenas to the two minibatch tensors, with nothing drawn on the host but `seed`:
 *   img, seg  : fp32 [n][t][hs][ws] depth / mask arenas, n = horizon * envs flat rows; either may be NULL (absent: its planes
 *               are not launched and its output is not looked at), not both; never written
 *   rows      : [b] flat rows (the ones igi_gather_rows takes); one outside [0, n) reads as frames of zeros
 *   the output is at the stored size (no crop).  Per (sample, tensor) one angle in +- max_rad radians shared by its t frames
 *   (max_rad == 0: no rotation, no hash) and, with masking_prob > 0, per depth frame the keep value of every hs / patch x
 *   ws / patch patch (kept with probability 1 - masking_prob) are the counter hash of (seed, site, element) at the sites
 *   tabled in csrc/augment_seeded.h, every event an integer comparison.  Only the depth frames are masked
 *   noise_std : as igi_image_pair_augment, from the same seed, on both tensors
 *   out_img, out_seg : fp32 [b][t][hs][ws], no arena; hs * ws above 2^24: IGI_E_BADARG; more than 8192 patches per frame:
 *               IGI_E_UNSUPPORTED
 *   draws     : int32 [b][2] or NULL: the fp32 bit patterns of the depth and the mask angle of every sample (both, whichever
 *               arena is present).  masking_prob outside [0, 1], or > 0 with patch < 1; max_rad negative or NaN: IGI_E_BADARG.
 *               Same arguments, same bits
 * ---------------------------------------------------------------------------------------- */
int igi_image_pair_augment_seeded(const float* img, const float* seg, int64_t n, int t, int hs, int ws, const int64_t* rows,
                                  int64_t b, int patch, float noise_std, double masking_prob, float max_rad, uint64_t seed,
                                  float* out_img, float* out_seg, int32_t* draws, igi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-time augmentation of the online student's segmented point cloud (csrc/pcl_augment.h), ONE launch from the
 * environment's cloud tensor to a new tensor (PointCloudAugmentations.augment of the reference's environment,
 * factory_utils.py:83-166, which runs it object by object on a boolean-masked subset of the envs):
 *   clouds    : fp32 [n][p_total][3], p_total = the sum of points[0 .. nobj), nobj in 1..4 consecutive objects (the layout
 *               of igi_pointnet_forward_multi); never written.  points[o] in 1..4096 (above: IGI_E_UNSUPPORTED)
 *   points    : HOST array of nobj counts
 *   episode   : DEVICE int32 [n], the caller's episode counter of every env; never written
 *   params    : the stages' parameters.  Env e is augmented iff its hit draw falls below hit_prob (one draw per env); a
 *               missed env is copied bit for bit.  A hit cloud: (a) x += clamp(sigma z, +-noise_clip) on the points whose
 *               mask draw falls below noise_prob, then x += clamp(const_noise pn, +-noise_clip); (b) rot_deg > 0: rotation
 *               about one axis through the origin by an angle uniform in +-rot_deg degrees; (c) int(points[o] *
 *               outlier_ratio) points replaced by outliers -- with probability contour_prob just outside the cloud's
 *               bounding box, else outlier_scale z; of two outliers on one point the later one wins; (d) dropout_ratio > 0:
 *               with probability 1 - no_dropout_prob per cloud, every point is zeroed with probability dropout_ratio.
 *               pn, the angle and the axis are per-episode: a pure function of (seed_episode, env, episode[env]), shared
 *               by an env's objects; every other draw is a pure function of (seed_step, element).  The hash sites and
 *               Gaussian planes are tabled in csrc/pcl_augment.h.  Probabilities outside [0, 1], negative sigma /
 *               noise_clip / rot_deg / ratios, and n * p_total * 3 >= 2^32: IGI_E_BADARG
 *   out       : fp32 [n][p_total][3], not the input.  Same arguments, same bits
 * ---------------------------------------------------------------------------------------- */
#define IGI_PCL_AUG_MAX_POINTS 4096
typedef struct igi_pcl_augment_params {
  double sigma, noise_clip, const_noise, noise_prob, hit_prob, rot_deg, outlier_ratio, contour_prob, outlier_scale,
      dropout_ratio, no_dropout_prob;
} igi_pcl_augment_params;
int igi_pcl_augment(const float* clouds, int64_t n, int nobj, const int32_t* points, const int32_t* episode,
                    const igi_pcl_augment_params* params, uint64_t seed_episode, uint64_t seed_step, float* out,
                    igi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IGI_PPO_H */
