"""The heads + PPO loss + head backward stage (csrc/ppo_loss.h: k_trunk_loss, k_loss_packed<1|2|4>, k_loss<1|2|4>) OFF the
freshly initialised policy, against a float64 restatement of the same minibatch (tests/loss_branch_cases.py).

Every other update test starts where the old policy is the current one, sigma = 0, mu stays far inside the soft bound and
entropy_coef = 0: there x / var = x / sig, logstd[q] = logstd[0], blo = 0, hardly a sample is clipped and the entropy term
of d_sigma is zero, so none of those can be told from its wrong neighbour.  Here every action dimension has its own sigma,
every clipped branch of both losses holds >= 3 % of each minibatch for either sign, mu > 1.1 on >= 5 % of the entries, and
all four coefficients differ from their defaults -- asserted from the float64 reference before anything is launched, with
no sample within 1e-4 of a kink of the gradient (so the fp32 kernels take the reference's branch for every sample and no
sample is excused).

Per case the first mini-epoch is walked FORCED: before each step the engine is given the oracle's parameters and Adam
moments, then fwd_bwd, compare, apply, compare.  Bounds (the project's single-step bounds, none widened):
  gradient ............. PER TENSOR, on the tensor's own scale: atol 2e-4 max|ref tensor|, rtol 2e-3 (the step-0 bound of
                         test_gpu_teacher_shapes.py, there on the scale of the whole gradient; per tensor as it holds the contact
                         encoder); sigma, mu.weight, mu.bias, value.weight, value.bias by name, each with a non-zero reference
  actor / critic / bounds / entropy means .. rtol 2e-4, atol 2e-6;  KL rtol 2e-3, atol 1e-7
  clip norm rtol 1e-3 (against the float64 gradient's norm), parameter norm rtol 1e-5
  written-back mus atol 2e-5, sigmas rtol 1e-5 (one sigma per action dimension: a real per-dimension check here)
  parameters after apply atol 0.1 lr
Which kernel ran is asserted through the profiler's classes; within "k_loss" the instantiation follows from act and
ceil(units[-1] / 64) (loss_stage), which the case table restates and test_loss_branches_cpu.py checks."""
import numpy as np
import pytest
import torch

from tests import loss_branch_cases as L

pytestmark = pytest.mark.gpu

HEADS = ("sigma", "mu.weight", "mu.bias", "value.weight", "value.bias")


def _assert_conditions(case, slot, ref):
    classes, mu_share = L.census(ref)
    for nm, share in classes.items():
        assert share >= L.CLASS_FLOOR, (case, slot, nm, share)
    assert mu_share >= L.MU_FLOOR, (case, slot, mu_share)
    assert L.near_kink(ref) == 0, (case, slot)


@pytest.mark.parametrize("case", list(L.CASES))
def test_loss_stage_off_policy_matches_float64(case):
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    (N, T, E), act, units, cls, inst, _, _, hp = L.CASES[case]
    w = L.walk(case)
    for slot, s in enumerate(w.steps):              # before anything is launched
        _assert_conditions(case, slot, s.ref)
    eng = TeacherEngine(N, T, E, units=units, priv_units=L.PRIV_UNITS, perm=w.perm, obs_dim=L.OBS, act_dim=act, **hp)
    eng.load_params(w.init)
    eng.prepare(w.ro)
    names = list(w.init)
    other = "k_loss" if cls == "k_trunk_loss" else "k_trunk_loss"
    failures = []

    def close(got, want, what, **tol):
        try:
            np.testing.assert_allclose(got, want, err_msg=what, **tol)
        except AssertionError as e:
            failures.append(str(e))

    for slot, s in enumerate(w.steps):
        # force: the step starts from the oracle's parameters and Adam moments
        eng.load_params(s.params)
        mv, vv = eng.param_views(eng.adam_m), eng.param_views(eng.adam_v)
        for k, (m_, v_) in s.adam.items():
            mv[k].copy_(m_)
            vv[k].copy_(v_)
        _lib.prof_enable(True)
        try:
            eng.fwd_bwd(slot, slot)
            torch.cuda.synchronize()
            classes = {}
            for c in _lib.prof_read():
                nm = c["name"].split(":")[0]
                classes[nm] = classes.get(nm, 0) + c["launches"]
        finally:
            _lib.prof_enable(False)
        assert classes.get(cls, 0) == 1 and classes.get(other, 0) == 0, (case, inst, classes)
        # ---- gradient, per tensor on its own scale
        gv = {k: v.cpu().numpy() for k, v in eng.param_views(eng.grads).items()}
        off = 0
        for k in names:
            n = w.init[k].numel()
            r = s.ref.grad[off:off + n].reshape(w.init[k].shape).numpy()
            off += n
            rmax = np.abs(r).max()
            if k in HEADS:
                assert rmax > 0, (case, slot, k)
            print(f"{case} step {slot} {k}: max |diff| / max |ref| = {np.abs(gv[k] - r).max() / max(rmax, 1e-300):.2e}")
            close(gv[k], r, f"{case} step {slot}: gradient of {k}", atol=2e-4 * rmax, rtol=2e-3)
        eng.apply(slot)
        torch.cuda.synchronize()
        # ---- statistics row
        st = eng.stats[slot].cpu().numpy()
        for j, nm in enumerate(["a_loss", "c_loss", "b_loss", "entropy"]):
            close(st[j], s.ref.means[j], f"{case} step {slot}: {nm}", rtol=2e-4, atol=2e-6)
        if hp["bounds_loss_coef"] == 0:
            # frozen_ppo.py:554-560: no bounds term without a positive coefficient -- the statistic is 0, like the oracle's
            assert s.b_loss32 == 0.0
            close(st[2], 0.0, f"{case} step {slot}: b_loss under a zero coefficient", rtol=0, atol=0)
        close(st[4], s.ref.means[4], f"{case} step {slot}: KL", rtol=2e-3, atol=1e-7)
        close(st[5], s.ref.grad.norm().item(), f"{case} step {slot}: clip norm", rtol=1e-3)
        close(st[6], s.param_norm, f"{case} step {slot}: parameter norm", rtol=1e-5)
        # ---- update_mu_sigma of this minibatch's rows
        rows = s.ref.rows.numpy()
        close(eng.env_major(eng.mus_w).cpu().numpy()[rows], s.ref.mu.numpy(), f"{case} step {slot}: mus_w", atol=2e-5, rtol=0)
        close(eng.env_major(eng.sigmas_w).cpu().numpy()[rows], s.ref.sigma.numpy(), f"{case} step {slot}: sigmas_w", rtol=1e-5)
        # ---- one Adam step on the clipped gradient
        close(eng.packed().cpu().numpy(), s.params_after.numpy(), f"{case} step {slot}: parameters after apply",
              atol=0.1 * w.lr, rtol=0)
    # one mini-epoch visits every row once: the whole arena holds the oracle's scattered mus / sigmas
    assert E * eng.mb == eng.B
    close(eng.env_major(eng.mus_w).cpu().numpy(), w.mus.numpy(), f"{case}: mus_w after the mini-epoch", atol=2e-5, rtol=0)
    close(eng.env_major(eng.sigmas_w).cpu().numpy(), w.sigmas.numpy(), f"{case}: sigmas_w after the mini-epoch", rtol=1e-5)
    assert not failures, f"{len(failures)} comparison(s) failed:\n" + "\n".join(failures)
