// The packed teacher configuration of the mi355ppo ops, (int[] icfg, float[] fcfg), decoded ONCE: the layout below is
// the only place that knows where a field sits, and igi_teacher_cfg_unpack (igi_capi.hip) is the only decoder -- ops.py,
// torch_ops.cpp and C++ hosts call it and read named fields of the struct.  Host code only: the C headers and the ABI
// header, no HIP (tools/teacher_cfg_check.cpp compiles it with plain g++ under the sanitizers).
//
//   ints   : obs_dim, priv_dim, act_dim, n_priv_layers, priv_units[M], n_layers, units[M], num_envs, horizon, mini_epochs
//            then ONE of: nothing (plain) | 1, 0 (shared actor-critic trunk) | contact_points, contact_emb, only_contact
//            then, with the adaptive learning-rate schedule, lr_schedule (= 1)
//            then, with KL early stopping, kl_early_stop (= 1)
//   floats : gamma, tau, lr, beta1, beta2, adam_eps, e_clip, critic_coef, entropy_coef, bounds_loss_coef, grad_norm, rms_eps
//            then, with the schedule, kl_threshold, lr_min, lr_max;  then, with early stopping, its kl_threshold
// The lists carry no field names: the float count tells schedule and stop tail, the int count that remains the mode.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/igi_ppo.h"

enum {  // icfg
  TCI_OBS_DIM, TCI_PRIV_DIM, TCI_ACT_DIM, TCI_N_PRIV_LAYERS,
  TCI_PRIV_UNITS,
  TCI_N_LAYERS = TCI_PRIV_UNITS + IGI_MAX_LAYERS,
  TCI_UNITS,
  TCI_NUM_ENVS = TCI_UNITS + IGI_MAX_LAYERS, TCI_HORIZON, TCI_MINI_EPOCHS,
  TCI_N_PLAIN,                                                                       // a plain teacher ends here
  TCI_SHARED = TCI_N_PLAIN, TCI_SHARED_ZERO, TCI_N_SHARED,                           // the pair (1, 0)
  TCI_CONTACT_POINTS = TCI_N_PLAIN, TCI_CONTACT_EMB, TCI_ONLY_CONTACT, TCI_N_CONTACTS,
};
enum {  // fcfg
  TCF_GAMMA, TCF_TAU, TCF_LR, TCF_BETA1, TCF_BETA2, TCF_ADAM_EPS, TCF_E_CLIP, TCF_CRITIC_COEF, TCF_ENTROPY_COEF,
  TCF_BOUNDS_LOSS_COEF, TCF_GRAD_NORM, TCF_RMS_EPS,
  TCF_N_FIXED,
  TCF_KL_THRESHOLD = TCF_N_FIXED, TCF_LR_MIN, TCF_LR_MAX, TCF_N_SCHED,
};

// Decodes and validates both lists.  ks == NULL: lists with the early-stopping tail are refused like any other wrong
// length.  ks != NULL: it is zeroed, and a tail fills kl_early_stop / kl_threshold (stop_state stays NULL: the caller owns
// the tensor).  Returns the number of optimizer steps the stop record covers, E * (B / (B / E)) with B = num_envs * horizon
// (0 without a tail), or IGI_E_BADARG with the reason in err.
static inline int64_t igi_teacher_cfg_decode(const int64_t* icfg, int n_int, const double* fcfg, int n_float,
                                             igi_teacher_cfg* c, igi_kl_stop* ks, char* err, size_t err_len) {
#define TC_REFUSE(...) do { snprintf(err, err_len, __VA_ARGS__); return IGI_E_BADARG; } while (0)
  if (err_len) err[0] = 0;
  if (!c || n_int < 0 || n_float < 0 || (n_int && !icfg) || (n_float && !fcfg)) TC_REFUSE("teacher cfg: null argument");
  memset(c, 0, sizeof(*c));
  if (ks) memset(ks, 0, sizeof(*ks));
  const int stop = ks && (n_float == TCF_N_FIXED + 1 || n_float == TCF_N_SCHED + 1);
  if (stop) {   // the tail rides behind everything else: checked first, then taken off
    if (n_int < 1 || icfg[n_int - 1] != 1 || !(fcfg[n_float - 1] > 0))
      TC_REFUSE("teacher cfg: the early-stopping tail needs kl_early_stop == 1, kl_threshold > 0 and the stop_state tensor "
                "behind the state list");
    ks->kl_early_stop = 1; ks->kl_threshold = fcfg[n_float - 1];
    --n_int; --n_float;
    if (n_int < TCI_N_PLAIN) TC_REFUSE("teacher cfg: too short for the early-stopping tail");
  }
  const int sched = n_float == TCF_N_SCHED;   // + lr_schedule | kl_threshold, lr_min, lr_max
  const int ni = n_int - sched;
  if ((ni != TCI_N_PLAIN && ni != TCI_N_SHARED && ni != TCI_N_CONTACTS) || (n_float != TCF_N_FIXED && !sched))
    TC_REFUSE("teacher cfg: expected %d (%d with a shared trunk, %d with contacts) ints and %d floats (one more int and %d "
              "floats with the adaptive learning-rate schedule), got %d and %d", TCI_N_PLAIN, TCI_N_SHARED, TCI_N_CONTACTS,
              TCF_N_FIXED, TCF_N_SCHED, n_int, n_float);
  for (int i = 0; i < n_int; ++i)   // range first, then narrow
    if (icfg[i] < INT32_MIN || icfg[i] > INT32_MAX) TC_REFUSE("teacher cfg: int %d (%lld) does not fit 32 bits", i, (long long)icfg[i]);
  if (sched) {
    c->lr_schedule = (int32_t)icfg[ni];
    c->kl_threshold = fcfg[TCF_KL_THRESHOLD]; c->lr_min = fcfg[TCF_LR_MIN]; c->lr_max = fcfg[TCF_LR_MAX];
    if (c->lr_schedule != 1 || !(c->kl_threshold > 0) || !(c->lr_min > 0) || !(c->lr_min <= c->lr_max))
      TC_REFUSE("teacher cfg: the schedule fields need lr_schedule == 1, kl_threshold > 0 and 0 < lr_min <= lr_max");
  }
  c->obs_dim = (int32_t)icfg[TCI_OBS_DIM]; c->priv_dim = (int32_t)icfg[TCI_PRIV_DIM]; c->act_dim = (int32_t)icfg[TCI_ACT_DIM];
  c->n_priv_layers = (int32_t)icfg[TCI_N_PRIV_LAYERS]; c->n_layers = (int32_t)icfg[TCI_N_LAYERS];
  for (int i = 0; i < IGI_MAX_LAYERS; ++i) {
    c->priv_units[i] = (int32_t)icfg[TCI_PRIV_UNITS + i]; c->units[i] = (int32_t)icfg[TCI_UNITS + i];
  }
  c->num_envs = (int32_t)icfg[TCI_NUM_ENVS]; c->horizon = (int32_t)icfg[TCI_HORIZON]; c->mini_epochs = (int32_t)icfg[TCI_MINI_EPOCHS];
  if (ni == TCI_N_CONTACTS) {
    c->contact_points = (int32_t)icfg[TCI_CONTACT_POINTS]; c->contact_emb = (int32_t)icfg[TCI_CONTACT_EMB];
    c->only_contact = (int32_t)icfg[TCI_ONLY_CONTACT];
    if (c->contact_points < 1) TC_REFUSE("teacher cfg: the contact fields need contact_points >= 1");
  }
  if (ni == TCI_N_SHARED) {
    c->shared_parameters = (int32_t)icfg[TCI_SHARED];
    if (c->shared_parameters != 1 || icfg[TCI_SHARED_ZERO] != 0) TC_REFUSE("teacher cfg: the shared-trunk fields must be (1, 0)");
  }
  c->gamma = fcfg[TCF_GAMMA]; c->tau = fcfg[TCF_TAU];
  c->lr = fcfg[TCF_LR]; c->beta1 = fcfg[TCF_BETA1]; c->beta2 = fcfg[TCF_BETA2]; c->adam_eps = fcfg[TCF_ADAM_EPS];
  c->e_clip = (float)fcfg[TCF_E_CLIP]; c->critic_coef = (float)fcfg[TCF_CRITIC_COEF];
  c->entropy_coef = (float)fcfg[TCF_ENTROPY_COEF]; c->bounds_loss_coef = (float)fcfg[TCF_BOUNDS_LOSS_COEF];
  c->grad_norm = (float)fcfg[TCF_GRAD_NORM]; c->rms_eps = (float)fcfg[TCF_RMS_EPS];
  if (c->obs_dim < 1 || c->priv_dim < 1 || c->act_dim < 1 || c->num_envs < 1 || c->horizon < 1 || c->mini_epochs < 1 ||
      c->n_layers < 1 || c->n_layers > IGI_MAX_LAYERS || c->n_priv_layers < 1 || c->n_priv_layers > IGI_MAX_LAYERS)
    TC_REFUSE("teacher cfg: non-positive dimension or unsupported layer count");
  if (!stop) return 0;
  const int64_t B = (int64_t)c->num_envs * c->horizon, E = c->mini_epochs;
  if (B < E) TC_REFUSE("teacher cfg: non-positive dimension or unsupported layer count");
  if (sched && c->kl_threshold != ks->kl_threshold)      // one threshold: the scheduler's is the stop's
    TC_REFUSE("teacher cfg: the early-stopping tail's kl_threshold %.17g differs from the adaptive schedule's %.17g",
              ks->kl_threshold, c->kl_threshold);
  return E * (B / (B / E));
#undef TC_REFUSE
}
