"""The conditions of tests/loss_branch_cases.py on the CPU: for every case test_gpu_loss_branches.py compares and every
minibatch of its first mini-epoch, the off-policy problem really populates every branch of the clipped losses and the
upper side of the bounds term, no sample sits on a kink of the gradient, and the float64 restatement the GPU is compared
with is the fp32 oracle's own gradient (itself pinned to the reference's goldens) up to fp32 rounding.  These are
conditions on the test data, not measurements of the product: a case or seed that stops meeting them fails here (and in the
GPU test before it launches anything), instead of turning a comparison vacuous."""
import math

import pytest
import torch

from tests import loss_branch_cases as L


def test_the_problem_is_off_the_initial_policy():
    """What teacher_problem hides, present: distinct sigmas (none 1), a mu head that reaches the soft bound, non-zero
    mu.bias and trunk biases, old mus / sigmas / values that are not the network's, neglogpacs that are the old policy's."""
    from oracle import synth, teacher as ot
    (N, T, E), act, units, _, _, seed, force, _ = L.CASES["packed2_act7"]
    base, ro0, perm0 = synth.teacher_problem(N, T, units, L.PRIV_UNITS, act_dim=act, seed=seed, done_p=0.1)
    init, ro, perm = L.off_policy_problem(N, T, units, L.PRIV_UNITS, act, seed)
    sig = torch.exp(init["sigma"])
    assert torch.equal(init["sigma"].sort().values, torch.linspace(-0.7, 0.4, act))
    assert len(set(init["sigma"].tolist())) == act and (sig - 1.0).abs().min() > 0.03
    assert torch.equal(init["mu.weight"], base["mu.weight"] * 100.0) and not init["value.bias"].any()
    assert init["mu.bias"].abs().min() > 0
    for k, v in init.items():
        assert v.shape == base[k].shape
        if "_mlp." in k:
            assert (v.abs().max() > 0) if k.endswith("bias") else torch.equal(v, base[k]), k
    assert torch.equal(perm, perm0)
    for k in ("obses", "priv_info", "rewards", "dones", "last_values"):
        assert torch.equal(ro[k], ro0[k]), k
    for k in ("mus", "sigmas", "actions", "neglogpacs", "values"):
        assert ro[k].shape == ro0[k].shape and not torch.equal(ro[k], ro0[k]), k
    # one old sigma per action dimension, off the current one; neglogpacs belong to the OLD policy
    s_old = ro["sigmas"].reshape(-1, act)
    assert torch.equal(s_old, s_old[:1].expand_as(s_old)) and ((s_old[0] / sig).log().abs() > 1e-3).all()
    nlp = ot.gaussian_neglogp(ro["actions"], ro["mus"], ro["sigmas"], torch.log(ro["sigmas"]))
    assert torch.equal(nlp, ro["neglogpacs"])
    # the fallback for a case that cannot reach mu > 1.1 otherwise: alternate signs, the same magnitudes
    forced, _, _ = L.off_policy_problem(N, T, units, L.PRIV_UNITS, act, seed, force_bias_sign=True)
    assert torch.equal(forced["mu.bias"].abs(), init["mu.bias"].abs())
    assert forced["mu.bias"].sign().tolist() == [1.0 if q % 2 == 0 else -1.0 for q in range(act)]


def test_case_table_names_the_kernel_each_shape_selects():
    for name, ((N, T, E), act, units, cls, inst, _, _, _) in L.CASES.items():
        assert L.expected_instantiation(act, units) == inst, name
        assert cls == ("k_trunk_loss" if inst == "k_trunk_loss" else "k_loss"), name
    assert {c[4] for c in L.CASES.values()} == {"k_trunk_loss"} | {f"k_loss{p}<{j}>" for p in ("", "_packed") for j in (1, 2, 4)}


@pytest.mark.parametrize("case", list(L.CASES))
def test_conditions_hold_on_every_compared_minibatch(case):
    w = L.walk(case)
    (N, T, E), act, units = L.CASES[case][:3]
    assert len(w.steps) == E and all(s.ref.rows.numel() == N * T // E for s in w.steps)
    for slot, s in enumerate(w.steps):
        classes, mu_share = L.census(s.ref)
        kinks = L.near_kink(s.ref)
        err = ((s.grad32.double() - s.ref.grad).abs().max() / s.ref.grad.abs().max()).item()
        print(f"{case} minibatch {slot}: smallest class {min(classes.values()):.3f}, mu > 1.1 {mu_share:.3f}, "
              f"near_kink {kinks}, oracle vs float64 {err:.1e} of the largest entry, |grad| {s.ref.grad.norm().item():.2f}")
        for nm, share in classes.items():
            assert share >= L.CLASS_FLOOR, (case, slot, nm, share)
        assert mu_share >= L.MU_FLOOR, (case, slot, mu_share)
        assert kinks == 0, (case, slot, kinks)
        assert err <= 1e-5, (case, slot, err)
        # the oracle's zero-coefficient branch (oracle/teacher.py: b_loss = zeros) against the restatement's
        if w.hp["bounds_loss_coef"] == 0:
            assert s.b_loss32 == 0.0 and s.ref.means[2] == 0.0
        else:
            assert s.b_loss32 > 0 and math.isclose(s.b_loss32, s.ref.means[2], rel_tol=1e-5)
