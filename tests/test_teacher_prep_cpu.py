"""CPU checks of what test_gpu_teacher_prep.py stands on: the float64 restatement (tests/teacher_prep_ref.py) against the
fp32 CPU oracle on the data the oracle is pinned on, the oracle's own error on the column kinds of
tests/teacher_prep_cases.py (finite, printed: the GPU bounds are 3 x it or an fp32 floor, whichever is larger), and the
conditions under which the GPU comparisons mean something -- (gamma, tau) pairs whose product rounds differently in the
two orders, tail columns that clamp on both sides, constant columns of variance exactly 0, a loss that moves when the clamp
is taken out."""
import numpy as np
import pytest
import torch

from tests import teacher_prep_cases as tc
from tests import teacher_prep_ref as tr


def _f32(x):
    return np.float32(x)


def _states_agree(got, want):
    """1e-6 relative: the var to itself, the mean to the column's scale |mean| + std (a mean of centred data has no scale
    of its own: the fp32 batch mean of N(0, 1) rows is off by 2^-24 of the entries it sums, not of their mean)."""
    scale = want.mean.abs() + want.var.sqrt()
    assert ((got.mean - want.mean).abs() <= 1e-6 * scale).all(), ((got.mean - want.mean).abs() / scale).max()
    np.testing.assert_allclose(got.var.numpy(), want.var.numpy(), rtol=1e-6)
    assert got.count.item() == want.count.item()


def test_gamma_tau_pairs_tell_the_two_rounding_orders_apart():
    """teacher_prepare forms (float)(gamma * tau) in double, as gamma * tau * nn * lam does in the reference (Python
    doubles times an fp32 tensor).  A kernel that multiplied the two fp32 values passes wherever the orders agree."""
    differ = [(g, t) for g, t in tc.GAE_PAIRS if _f32(g * t) != _f32(g) * _f32(t)]
    print("pairs whose orders differ:", differ)
    assert len(differ) >= 2 and (0.9, 0.8) in differ and (0.998, 0.95) in differ
    assert _f32(0.99 * 0.95) == _f32(0.99) * _f32(0.95)          # the default pair cannot tell them apart
    assert {c[3] for c in tc.CASES.values()} == set(tc.GAE_PAIRS)   # every pair is some case's


def test_every_kind_is_in_both_inputs():
    for name, (_, obs_dim, priv_dim, _, _, _) in tc.CASES.items():
        assert set(tc.obs_kinds(obs_dim)) == set(tc.KINDS) == set(tc.priv_kinds(priv_dim)), name


@pytest.mark.parametrize("N,T,E", [(64, 8, 2), (37, 5, 5)])
def test_restatement_agrees_with_the_oracle_on_unit_normal_data(N, T, E):
    """synth.teacher_problem: TeacherOracle.prepare and RmsState against the restatement -- states 1e-6 relative, rows
    2e-5 (the suite's bounds for this stage, test_gpu_edges.py)."""
    from oracle import synth, teacher as ot
    init, ro, perm = synth.teacher_problem(N, T, tc.UNITS, tc.PRIV_UNITS, seed=5, done_p=0.05)
    orc = ot.TeacherOracle(init, perm, N, T, E, tc.UNITS, tc.PRIV_UNITS)
    d = orc.prepare(ro)
    p64 = tr.prepare64(ro, tr.State64.fresh(1), orc.hp["gamma"], orc.hp["tau"], 1e-5)
    np.testing.assert_allclose(orc.returns_raw.numpy(), p64.returns_raw.numpy(), atol=2e-5)
    np.testing.assert_allclose(d["advantages"].numpy(), p64.advantages.numpy(), atol=2e-5)
    np.testing.assert_allclose(d["values"].numpy(), p64.values_n.numpy(), atol=2e-5)
    np.testing.assert_allclose(d["returns"].numpy(), p64.returns_n.numpy(), atol=2e-5)
    _states_agree(tr.oracle_state(orc.rms_val), p64.rms_value)
    assert orc.rms_val.count.item() == p64.rms_value.count.item() == 1 + 2 * N * T
    mb = N * T // E
    t64 = tr.trajectory64(ro, perm, E, mb, tr.State64.fresh(15), tr.State64.fresh(64), 1e-5)
    t32 = tr.oracle_trajectory(ro, perm, E, mb, tr.State64.fresh(15), tr.State64.fresh(64), 1e-5)
    assert len(t64) == len(t32) == E * (N * T // mb)
    for a, b in zip(t64, t32):
        for sa, sb in ((a.obs_state, b.obs_state), (a.priv_state, b.priv_state)):
            _states_agree(sb, sa)
        np.testing.assert_allclose(b.obs.numpy(), a.obs.numpy(), atol=2e-5)
        np.testing.assert_allclose(b.priv.numpy(), a.priv.numpy(), atol=2e-5)
    # un-normalise is normalise's inverse inside the clamp
    st = t64[-1].obs_state
    y = st.normalize(t64[-1].raw_obs, 1e-5)
    inside = y.abs() < 5.0
    np.testing.assert_allclose(st.unnormalize(y, 1e-5)[inside].numpy(), t64[-1].raw_obs[inside].numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_oracle_error_on_the_column_kinds_is_finite(name):
    """The fp32 oracle against the restatement on every generator case, per column kind: finite, and printed (these are
    the (b) terms of the GPU bounds)."""
    c = tc.case(name)
    kinds = tc.obs_kinds(c["obs_dim"]) + tc.priv_kinds(c["priv_dim"])
    fresh = (tr.State64.fresh(c["obs_dim"]), tr.State64.fresh(c["priv_dim"]))
    t64 = tr.trajectory64(c["ro"], c["perm"], c["E"], c["mb"], *fresh, c["rms_eps"])
    t32 = tr.oracle_trajectory(c["ro"], c["perm"], c["E"], c["mb"], *fresh, c["rms_eps"])
    worst = {k: [0.0, 0.0, 0.0] for k in tc.KINDS}
    for a, b in zip(t64, t32):
        em = torch.cat([(b.obs_state.mean - a.obs_state.mean).abs(), (b.priv_state.mean - a.priv_state.mean).abs()])
        ev = torch.cat([(b.obs_state.var - a.obs_state.var).abs() / a.obs_state.var.clamp_min(1e-300),
                        (b.priv_state.var - a.priv_state.var).abs() / a.priv_state.var.clamp_min(1e-300)])
        er = torch.cat([(b.obs.double() - a.obs).abs().amax(0), (b.priv.double() - a.priv).abs().amax(0)])
        assert torch.isfinite(em).all() and torch.isfinite(ev).all() and torch.isfinite(er).all()
        for j, k in enumerate(kinds):
            w = worst[k]
            w[0], w[1], w[2] = max(w[0], float(em[j])), max(w[1], float(ev[j])), max(w[2], float(er[j]))
    for k, w in worst.items():
        print(f"{name:8s} {k:7s} oracle error: mean {w[0]:.2e} abs, var {w[1]:.2e} rel, rows {w[2]:.2e} abs")
    p64 = tr.prepare64(c["ro"], tr.State64.fresh(1), c["gamma"], c["tau"], c["rms_eps"])
    p32 = tr.oracle_prepare(c["ro"], tr.State64.fresh(1), c["gamma"], c["tau"], c["rms_eps"])
    for q in ("advantages", "values_n", "returns_n"):
        e = (getattr(p32, q).double() - getattr(p64, q)).abs().max()
        assert torch.isfinite(e)
        print(f"{name:8s} {q}: oracle error {float(e):.2e}")


@pytest.mark.parametrize("name", list(tc.CASES))
def test_tail_columns_clamp_on_both_sides_and_constant_columns_have_no_variance(name):
    c = tc.case(name)
    okinds, pkinds = tc.obs_kinds(c["obs_dim"]), tc.priv_kinds(c["priv_dim"])
    t64 = tr.trajectory64(c["ro"], c["perm"], c["E"], c["mb"], tr.State64.fresh(c["obs_dim"]),
                          tr.State64.fresh(c["priv_dim"]), c["rms_eps"])
    for kinds, rows in ((okinds, torch.cat([s.obs for s in t64])), (pkinds, torch.cat([s.priv for s in t64]))):
        for j, k in enumerate(kinds):
            if k == "tail":
                hi, lo = float((rows[:, j] == 5.0).double().mean()), float((rows[:, j] == -5.0).double().mean())
                print(f"{name} tail column {j}: {hi:.4f} clamped at +5, {lo:.4f} at -5")
                assert hi >= 0.005 and lo >= 0.005, (name, j, hi, lo)
            if k in ("const", "zero"):
                for s in t64:
                    x = s.raw_obs if kinds is okinds else s.raw_priv
                    n = x.shape[0]
                    assert float(((x[:, j] - x[:, j].mean()) ** 2).sum() / (n - 1)) == 0.0
    m, v, _ = tc.warm_state(okinds, c["T"], c["N"], seed=99)
    for j, k in enumerate(okinds):
        if k in ("const", "zero"):
            assert float(v[j]) == 0.0 and float(m[j]) == (float(np.float32(0.37)) if k == "const" else 0.0)


def test_the_step0_loss_notices_a_missing_clamp():
    """The float64 loss and gradient of step 0 fed UNCLAMPED rows move by more than 10 x the bounds the GPU test holds them
    to (2e-4 max|g| + 2e-3 |g| per gradient entry, 2e-4 relative on the critic loss)."""
    c = tc.case("mb300")
    hp = _hp()
    prep = tr.prepare64(c["ro"], tr.State64.fresh(1), c["gamma"], c["tau"], c["rms_eps"])
    fresh = (tr.State64.fresh(c["obs_dim"]), tr.State64.fresh(c["priv_dim"]))
    out = []
    for clamp in (True, False):
        s = tr.trajectory64(c["ro"], c["perm"], c["E"], c["mb"], *fresh, c["rms_eps"], clamp=clamp, steps=1)[0]
        out.append(tr.step_loss64(c["init"], s.obs, s.priv, s.idx, c["ro"], prep, hp, len(tc.PRIV_UNITS), len(tc.UNITS)))
    moved = tr.clamp_sensitivity(*out)
    print("clamp removed: (gradient move / bound, critic-loss move / bound) =", moved)
    assert moved[0] > 10.0 and moved[1] > 10.0


def _hp():
    from oracle.teacher import TeacherOracle
    return dict(TeacherOracle.HP)
