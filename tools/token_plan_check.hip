// Stand-alone host check of make_token_plan (csrc/token_encoder.h), meant for a sanitizer build; no kernel is launched:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/token_plan_check.hip \
//         -o token_plan_check && ./token_plan_check
//
// Sweeps batch 1 .. 8200 (coarse stride), seq 1 .. 33, layers 1 .. 9, ff in {4, 128, 130}, eval and train.  A plan that is
// accepted must have every offset 4-float aligned, every parameter offset inside a layer's parameters, every activation
// offset inside a layer's slab, and every slab / scratch region inside total_bytes; seq 33, layers 9 and ff 130 are refused.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../include/igi_ppo.h"
#include "../isaacgyminsertion_amd/csrc/gemm_dma.h"
#include "../isaacgyminsertion_amd/csrc/gemm_f32.h"
#include "../isaacgyminsertion_amd/csrc/rms.h"
#include "../isaacgyminsertion_amd/csrc/rollout.h"
#include "../isaacgyminsertion_amd/csrc/pointnet.h"
#include "../isaacgyminsertion_amd/csrc/tactile.h"
#include "../isaacgyminsertion_amd/csrc/teacher.h"
#include "../isaacgyminsertion_amd/csrc/linear.h"
#include "../isaacgyminsertion_amd/csrc/token_encoder.h"

int main() {
  long long plans = 0, refused = 0, bad = 0;
  const int ffs[3] = {4, 128, 130};
  for (int B = 1; B <= 8200; B += (B < 70 ? 1 : 271))
    for (int S = 1; S <= 33; ++S)
      for (int L = 1; L <= 9; ++L)
        for (int ff : ffs)
          for (int training = 0; training < 2; ++training) {
            igi_token_cfg c = {};
            c.batch = B; c.seq = S; c.d_model = 32; c.nhead = 2; c.ff = ff; c.layers = L; c.dropout = 0.1f; c.training = training;
            igi::TokenPlan p;
            const int rc = igi::make_token_plan(&c, &p);
            const bool want_refusal = S > 32 || L > 8 || ff == 130;
            if (rc) {
              ++refused;
              if (!want_refusal) { ++bad; printf("refused B %d S %d L %d ff %d: %d\n", B, S, L, ff, rc); }
              continue;
            }
            ++plans;
            const igi::TokLayout& y = p.lay;
            const long long o[12] = {y.o_inw, y.o_inb, y.o_ow, y.o_ob, y.o_w1, y.o_b1, y.o_w2, y.o_b2, y.o_n1w, y.o_n1b, y.o_n2w, y.o_n2b};
            const long long a[10] = {y.a_x, y.a_st1, y.a_xn1, y.a_qkv, y.a_ctx, y.a_x1, y.a_st2, y.a_xn2, y.a_z, y.a_h};
            const long long s[9] = {p.s_g0, p.s_g1, p.s_rA, p.s_rB, p.s_wide0, p.s_wide1, p.s_lnpart, p.s_part, p.s_lin};
            bool ok = !want_refusal && (y.per_layer & 3) == 0 && (y.a_layer & 3) == 0;
            for (long long v : o) ok = ok && v >= 0 && v < y.per_layer && (v & 3) == 0;
            for (long long v : a) ok = ok && v >= 0 && v < y.a_layer && (v & 3) == 0;
            for (long long v : s) ok = ok && v >= y.a_layer * L && (v & 3) == 0 && sizeof(float) * (size_t)v <= p.total_bytes;
            ok = ok && sizeof(float) * (size_t)p.s_lin + p.lin_bytes * 4 * (size_t)L + 64 == p.total_bytes;
            if (!ok) { ++bad; printf("bad plan B %d S %d L %d ff %d\n", B, S, L, ff); }
          }
  printf("token_plan_check: %lld plans, %lld refusals, %lld bad\n", plans, refused, bad);
  return bad ? 1 : 0;
}
