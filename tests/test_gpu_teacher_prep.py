"""The data-dependent front of the teacher update -- k_gae, k_prep_final, k_prep_norm, k_gather_stats, k_mb_moments,
k_rms_traj, the normalise half of gather_normalize_body, k_rms_coef, k_normalize (csrc/teacher.h) and the stand-alone
RunningMeanStd (csrc/rms.h) -- OFF unit-normal rollouts, against the float64 restatement of tests/teacher_prep_ref.py.

Inputs: tests/teacher_prep_cases.py (column kinds unit, offset, far, wide, tiny, const, zero, tail, flag, clock in both
obses and priv_info; rewards 1 + 0.1 z with values + 100; a second update on shifted data; normalisers that have seen 1e8 samples, or one minibatch).
Hyper-parameters off the defaults: (gamma, tau) in (0.9, 0.8), (0.998, 0.95), (1.0, 1.0), (0.95, 0.0) -- the first two round
gamma * tau differently in double and in fp32 --, rms_eps 1e-3, normalize_value False.  Shapes (N, T, E): (75, 4, 1)
(10 gather blocks, the last of 12 rows), (300, 3, 3) (two k_gae blocks, the second ragged), (37, 5, 5), and (75, 4, 2) with
obs 20 + priv 150 = 170 columns (second c0 pass of k_mb_moments, second lap of k_rms_traj); nets [64, 32] / [32, 8].

Bounds.  Every entry of every tensor is compared with the float64 truth; nothing is masked.  A bound is the larger of
(a) the cost of the fp32 operations the reference itself performs (stated beside each assert) and (b) 3 x the error of
the fp32 CPU oracle (oracle.teacher.RmsState / gae_returns / normalized_advantages) against the same truth on the same
input -- the suite's margin for "as good as the fp32 reference" (test_gpu_tactile.py, test_gpu_depth_scale.py).  (b) is
per column for rows and states, one number for advantages / values / returns; it never comes from the GPU's output.
Losses and gradients keep the suite's rtol 2e-4 (+ 2e-6) and 2e-4 max|g| + 2e-3 |g|, and inference
test_infer_matches_oracle's bounds, all against float64.

The floor of a running state.  The fp32 operations are the batch moments x.mean(0) / x.var(0), which round by
2^-24 |b_mean| and 2^-23 b_var; the merge is fp64.  State64 (teacher_prep_ref.py) carries those two roundings through the
merges to first order.  After ONE merge into the fresh state that is 2^-24 |mean| for the running mean and
2^-23 var + (2^-24 mean)^2 for the running var.  Written with the RUNNING mean at every step, the same two formulas cannot
be met by any implementation that forms an fp32 batch mean: where batch means cancel (a tail column: batch means of +-2.6,
running mean 0.03) an exactly rounded fp32 batch mean merged in fp64 -- emulated on the CPU -- is up to 11.2 x over
2^-24 |running mean| (rows37, priv column 44, step 5).  Under the formulas written that way the kernels' first failures were
1.678 (rows37), 1.922 (gae2) and 2.713 (wide170) for the mean -- the emulation's figures, digit for digit -- and 1.151 for the
var (wide170, warm, second update).  Against the carried floors that emulation sits at
0.40 - 0.73, so they are no looser than the rounding they describe.

Observed worst observed / bound on an MI355X (each test prints its own as "RATIO <case> <quantity> <value>"):

  case     running mean  running var  advantages  values_n  returns_n  rms_value mean / var  step-0 gradient
  mb300       0.464         0.725       0.462      0.333     0.344       0.790 / 0.129         0.001
  gae2        0.690         0.535       0.333      0.062     0.456       0.048 / 0.097         0.003
  rows37      0.715         0.465       0.332      0.333     0.333       0.069 / 0.155         0.001
  wide170     0.670         0.679       0.333      0.333     0.333       0.087 / 0.051         0.001
  (running mean / var: the worst over rms_obs and rms_priv, every step of both updates, from the fresh, the 1e8-sample
  and the one-minibatch state.  0.333 = the kernel's output is the oracle's, bit for bit.)

  stand-alone op   rows (train, eval, un-normalise)  state mean  state var
  300 x 10               0.422                         0.333       0.283
  16384 x 10             0.573                         0.336       0.331
  33 x 300               0.527                         0.636       0.587
  131072 x 1 far         0.297                         0.016       0.015

The running-state figures are those of the exactly rounded fp32 batch moments (the emulation above) to three digits: the
uncentred fp64 sums of k_gather_stats / k_mb_moments / k_rms_partial add nothing visible on the offset and far columns at
these sizes, and the kernels were left as they are."""
import numpy as np
import pytest
import torch

from tests import teacher_prep_cases as tc
from tests import teacher_prep_ref as tr

pytestmark = pytest.mark.gpu

NPL, NL = len(tc.PRIV_UNITS), len(tc.UNITS)


def _engine(c, perm=None, **hp):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    kw = dict(gamma=c["gamma"], tau=c["tau"], rms_eps=c["rms_eps"])
    kw.update(hp)
    eng = TeacherEngine(c["N"], c["T"], c["E"], units=tc.UNITS, priv_units=tc.PRIV_UNITS, perm=c["perm"] if perm is None else perm,
                        obs_dim=c["obs_dim"], priv_dim=c["priv_dim"], act_dim=tc.ACT, **kw)
    eng.load_params(c["init"])
    return eng


def _hp():
    from isaacgyminsertion_amd.teacher_native import DEFAULT_HP
    return dict(DEFAULT_HP)


def _check(tag, quantity, got, truth, bnd):
    """Every entry within its bound; prints the worst observed / bound."""
    got = got.detach().cpu().double().reshape(truth.shape)
    r = tr.worst_ratio(got, truth, bnd)
    print(f"RATIO {tag} {quantity} {r:.3f}")
    assert r <= 1.0, (tag, quantity, r)


def _unpack(packed):
    p = packed.detach().cpu().double()
    d = (p.numel() - 1) // 2
    return tr.State64(p[:d], p[d:2 * d], p[2 * d])


def _check_state(tag, name, packed, s64, s32):
    """A running state against the truth.  Floors: State64.e_mean / e_var, the roundings of the reference's fp32 batch
    mean (2^-24 |b_mean|) and batch var (2^-23 b_var) carried through the merges -- after one merge into the fresh state
    2^-24 |mean| and 2^-23 var + (2^-24 mean)^2.  Or 3 x the oracle's error, per column.  count: exact."""
    got = _unpack(packed)
    _check(tag, name + ".mean", got.mean, s64.mean, tr.bound(s64.e_mean, s32.mean - s64.mean, cols=True))
    _check(tag, name + ".var", got.var, s64.var, tr.bound(s64.e_var, s32.var - s64.var, cols=True))
    assert float(got.count) == float(s64.count), (tag, name, float(got.count), float(s64.count))


def _write_state(dst, s):
    dst.copy_(s.packed().to(dst.device))


# ---- 1. GAE, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_variant", [False, True], ids=["plain", "values+100"])
@pytest.mark.parametrize("gamma,tau", tc.GAE_PAIRS)
def test_gae_is_bit_exact_off_the_default_discount(gamma, tau, value_variant):
    """returns_raw == oracle.teacher.gae_returns: (0.9, 0.8) and (0.998, 0.95) tell (float)(gamma * tau) from
    (float)gamma * (float)tau (test_teacher_prep_cpu.py asserts it); with random dones; N = 300 (two k_gae blocks, the
    second ragged) and N = 37."""
    from oracle import teacher as ot
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    for N, T, E in ((300, 3, 3), (37, 5, 5)):
        init, ro, perm = tc.rollout(N, T, seed=31 + N, value_variant=value_variant, done_p=0.2)
        assert 0 < int(ro["dones"].sum()) < N * T
        eng = TeacherEngine(N, T, E, units=tc.UNITS, priv_units=tc.PRIV_UNITS, perm=perm, gamma=gamma, tau=tau)
        eng.load_params(init)
        eng.prepare(ro)
        torch.cuda.synchronize()
        ref = ot.gae_returns(ro["rewards"], ro["values"], ro["dones"], ro["last_values"], gamma, tau)
        assert torch.equal(eng.returns_raw.cpu(), ref), (N, T, gamma, tau)


# ---- 2. prepare against float64 -------------------------------------------------------------------------------------
def _value_state(c, state):
    if state == "fresh":
        return tr.State64.fresh(1)
    _, other, _ = tc.rollout(c["N"], c["T"], c["obs_dim"], c["priv_dim"], seed=777, value_variant=tc.CASES[c["name"]][5])
    v = other["values"].double().reshape(-1, 1)
    return tr.State64(v.mean(0), v.var(0), torch.tensor(1e8))


@pytest.mark.parametrize("state", ["fresh", "warm"])
@pytest.mark.parametrize("normalize_value", [True, False], ids=["normalize_value", "raw_values"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_prepare_matches_float64(name, normalize_value, state):
    c = dict(tc.case(name), name=name)
    ro = c["ro"]
    tag = f"{name}/{state}/{'nv' if normalize_value else 'raw'}"
    st0 = _value_state(c, state)
    eng = _engine(c, normalize_value=normalize_value)
    _write_state(eng.rms_value, st0)
    before = eng.rms_value.clone()
    eng.prepare(ro)
    torch.cuda.synchronize()
    p64 = tr.prepare64(ro, st0, c["gamma"], c["tau"], c["rms_eps"], normalize_value)
    p32 = tr.oracle_prepare(ro, st0, c["gamma"], c["tau"], c["rms_eps"])
    assert torch.equal(eng.returns_raw.cpu(), p32.returns_raw)
    # an advantage (adv - mean) / (std + 1e-8) in fp32: 2^-24 (|adv| + |mean|) / den + 3 * 2^-24 |y|, or 3 x the oracle's error
    _check(tag, "advantages", eng.env_major(eng.advantages), p64.advantages,
           tr.bound(tr.floor_norm(p64.adv_raw, p64.adv_mean, p64.adv_den, p64.advantages), p32.advantages.double() - p64.advantages))
    if not normalize_value:
        assert torch.equal(eng.values_n.cpu(), ro["values"]) and torch.equal(eng.returns_n.cpu(), p32.returns_raw)
        assert torch.equal(eng.rms_value, before)
        return
    # a normalised value / return (x - m) / d in fp32: 2^-24 (|x| + |m|) / d + 3 * 2^-24 |y| and the state's own floor
    # (State64.floor_norm), or 3 x the oracle's error
    for q, x, s in (("values_n", p64.values, p64.val_states[0]), ("returns_n", p64.returns, p64.val_states[1])):
        y = getattr(p64, q)
        _check(tag, q, eng.env_major(getattr(eng, q)), y,
               tr.bound(s.floor_norm(x, c["rms_eps"], y), getattr(p32, q).double() - y))
    _check_state(tag, "rms_value", eng.rms_value, p64.rms_value, p32.rms_value)


# ---- 3. the normaliser trajectory -----------------------------------------------------------------------------------
def _run_steps(eng, tag, t64, t32):
    k = 0
    for _ in range(eng.E):
        for i in range(eng.n_mb):
            eng.fwd_bwd(i, k)
            eng.apply(k)
            torch.cuda.synchronize()
            _check_state(f"{tag}/step{k}", "rms_obs", eng.rms_obs, t64[k].obs_state, t32[k].obs_state)
            _check_state(f"{tag}/step{k}", "rms_priv", eng.rms_priv, t64[k].priv_state, t32[k].priv_state)
            k += 1
    assert k == len(t64) == len(t32) == eng.E * eng.n_mb


def _input_states(c, state):
    """fresh: (0, 1, 1).  warm: count 1e8 with the moments of a different draw of the same column kinds.  seen: the same
    moments with a count of ONE minibatch -- the only start from which a minibatch's own variance shows in the state of an
    offset or far column (from the fresh state delta^2 swamps it, from 1e8 samples nothing moves)."""
    if state == "fresh":
        return tr.State64.fresh(c["obs_dim"]), tr.State64.fresh(c["priv_dim"])
    count = 1e8 if state == "warm" else float(c["mb"])
    return (tr.State64(*tc.warm_state(tc.obs_kinds(c["obs_dim"]), c["T"], c["N"], seed=555, count=count)),
            tr.State64(*tc.warm_state(tc.priv_kinds(c["priv_dim"]), c["T"], c["N"], seed=556, count=count)))


@pytest.mark.parametrize("state", ["fresh", "warm", "seen"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_normaliser_trajectory_matches_sequential_chan_merges(name, state):
    """After every fwd_bwd + apply of an update, rms_obs / rms_priv (what block 0 of the gather publishes) against a
    sequential Chan merge of exact two-pass minibatch moments, from a fresh, a warm and a one-minibatch state; then a second prepare +
    update on shifted(ro) that continues from that state; update() as a whole leaves the step-wise loop's state, bit for bit."""
    c = tc.case(name)
    ro, ro2 = c["ro"], tc.shifted(c["ro"])
    eng, whole = _engine(c), _engine(c)
    s0 = _input_states(c, state)
    for e in (eng, whole):
        _write_state(e.rms_obs, s0[0])
        _write_state(e.rms_priv, s0[1])
    args = (c["perm"], c["E"], c["mb"])
    tag = f"{name}/{state}"
    eng.prepare(ro)
    t64, t32 = tr.trajectory64(ro, *args, *s0, c["rms_eps"]), tr.oracle_trajectory(ro, *args, *s0, c["rms_eps"])
    _run_steps(eng, tag + "/first", t64, t32)
    eng.prepare(ro2)
    u64 = tr.trajectory64(ro2, *args, t64[-1].obs_state, t64[-1].priv_state, c["rms_eps"])
    u32 = tr.oracle_trajectory(ro2, *args, t32[-1].obs_state, t32[-1].priv_state, c["rms_eps"])
    _run_steps(eng, tag + "/second", u64, u32)
    for r in (ro, ro2):
        whole.prepare(r)
        whole.update()
    torch.cuda.synchronize()
    for k in ("rms_obs", "rms_priv", "rms_value", "params"):
        assert torch.equal(getattr(whole, k), getattr(eng, k)), k


# ---- 4. the normalised rows as the network sees them ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_step0_record_and_gradient_follow_the_normalised_rows(name):
    """The step-0 loss record and the step-0 gradient of every parameter against oracle.teacher.forward_train + the loss in
    float64, fed the restatement's normalised (and clamped) rows and its advantages / values / returns.  The float64
    gradient itself moves by more than 10 x its bound when the restatement does not clamp: a kernel that lost clamp5 fails."""
    c = tc.case(name)
    ro, hp = c["ro"], _hp()
    eng = _engine(c)
    eng.prepare(ro)
    eng.fwd_bwd(0, 0)
    got = eng.packed(eng.grads).cpu().double().numpy()
    eng.apply(0)                                  # the step's record is complete once the optimizer has run
    torch.cuda.synchronize()
    prep = tr.prepare64(ro, tr.State64.fresh(1), c["gamma"], c["tau"], c["rms_eps"])
    s0 = (tr.State64.fresh(c["obs_dim"]), tr.State64.fresh(c["priv_dim"]))
    ref = []
    for clamp in (True, False):
        s = tr.trajectory64(ro, c["perm"], c["E"], c["mb"], *s0, c["rms_eps"], clamp=clamp, steps=1)[0]
        ref.append(tr.step_loss64(c["init"], s.obs, s.priv, s.idx, ro, prep, hp, NPL, NL))
    moved = tr.clamp_sensitivity(*ref)
    print(f"RATIO {name} clamp-removed-move/bound gradient {moved[0]:.1f} critic {moved[1]:.1f}")
    assert moved[0] > 10.0, moved
    want = ref[0]
    rec = eng.stats[0, :4].cpu().double().numpy()
    print(f"{name} step-0 record {rec} float64 {want.means}")
    np.testing.assert_allclose(rec, np.array(want.means), rtol=2e-4, atol=2e-6)
    g = want.grad.numpy()
    gmax = np.abs(g).max()
    print(f"RATIO {name} step0-gradient {float((np.abs(got - g) / (2e-4 * gmax + 2e-3 * np.abs(g))).max()):.3f}")
    np.testing.assert_allclose(got, g, atol=2e-4 * gmax, rtol=2e-3)


# ---- 5. inference with the state the update left --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_inference_after_the_update_matches_float64(name):
    """infer(normalize=True) on held-out rows of the same column kinds (tail outliers included) against float64 with the
    restatement's final state and the engine's own updated parameters, at test_infer_matches_oracle's bounds;
    normalize=False on the pre-normalised rows gives the same."""
    c = tc.case(name)
    eng = _engine(c)
    eng.prepare(c["ro"])
    eng.update()
    torch.cuda.synchronize()
    s0 = (tr.State64.fresh(c["obs_dim"]), tr.State64.fresh(c["priv_dim"]))
    last = tr.trajectory64(c["ro"], c["perm"], c["E"], c["mb"], *s0, c["rms_eps"])[-1]
    obs, priv = tc.held_out_rows(77, c["obs_dim"], c["priv_dim"], seed=4242)
    on, pn = last.obs_state.normalize(obs, c["rms_eps"]), last.priv_state.normalize(priv, c["rms_eps"])
    assert (on.abs() == 5.0).any() and (pn.abs() == 5.0).any()        # the clamp acts on these rows
    params = {k: v.cpu() for k, v in eng.param_views().items()}
    mu, val, lat = tr.infer64(params, on, pn, NPL, NL)
    for normalize, (o_in, p_in) in ((True, (obs, priv)), (False, (on.float(), pn.float()))):
        if not normalize:
            mu, val, lat = tr.infer64(params, o_in, p_in, NPL, NL)
        m, v, l = eng.infer(o_in, p_in, want_latent=True, normalize=normalize)
        torch.cuda.synchronize()
        np.testing.assert_allclose(m.cpu().numpy(), mu.numpy(), atol=2e-6, rtol=1e-4)
        np.testing.assert_allclose(v.cpu().numpy(), val.numpy(), atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(l.cpu().numpy(), lat.numpy(), atol=2e-6, rtol=1e-4)


# ---- 6. the stand-alone RunningMeanStd ------------------------------------------------------------------------------
RMS_CASES = {"300x10": (300, 10, None), "16384x10": (16384, 10, None), "33x300": (33, 300, None),
             "131072x1_far": (131072, 1, "far")}


@pytest.mark.parametrize("name", list(RMS_CASES))
def test_standalone_running_mean_std_matches_float64(name):
    """Two train steps (the second on 2 x + 3 std), then eval and un-normalise on a third draw, against the restatement;
    eval and un-normalise leave the state untouched."""
    from isaacgyminsertion_amd.algo.models.running_mean_std import RunningMeanStd
    rows, D, kind = RMS_CASES[name]
    kinds = [kind] if kind else tc.kinds_for(D, 0)
    g = torch.Generator().manual_seed(rows + D)
    x1 = tc.columns(kinds, rows, 1, g)[:, 0]
    x2 = (2.0 * x1.double() + 3.0 * x1.double().std(0)).float()
    x3 = tc.columns(kinds, rows, 1, g)[:, 0]
    eps = 1e-5
    m = RunningMeanStd((D,)).cuda()
    s64, s32 = tr.State64.fresh(D), tr.oracle_rms(tr.State64.fresh(D), eps)
    m.train()
    for step, x in enumerate((x1, x2)):
        y = m(x.cuda())
        torch.cuda.synchronize()
        s64.merge(x)
        y64, y32 = s64.normalize(x, eps), s32(x, train=True)
        # (x - m) / d in fp32: 2^-24 (|x| + |m|) / d + 3 * 2^-24 |y| and the state's own floor (State64.floor_norm), or
        # 3 x the oracle's error in the column
        _check(f"rms/{name}/train{step}", "rows", y, y64, tr.bound(s64.floor_norm(x, eps, y64), y32.double() - y64, cols=True))
        _check_state(f"rms/{name}/train{step}", "state", m.packed, s64, tr.oracle_state(s32))
    m.eval()
    before = m.packed.clone()
    y64 = s64.normalize(x3, eps)
    _check(f"rms/{name}/eval", "rows", m(x3.cuda()), y64,
           tr.bound(s64.floor_norm(x3, eps, y64), s32.normalize(x3).double() - y64, cols=True))
    # d * clamp(v) + m in fp32: d and the product round (2 * 2^-24 |d c|), then m (2^-24 |m|) and the sum (2^-24 |out|),
    # on top of the state's own floor (e_mean, and e_var / 2d through d)
    v = (3.0 * torch.randn(rows, D, generator=g)).float()
    u64 = s64.unnormalize(v, eps)
    vc, d = v.double().clamp(-5.0, 5.0).abs(), s64.den(eps)
    floor = tr.U * (2.0 * d * vc + s64.mean.abs() + u64.abs()) + s64.e_mean + s64.e_var / (2.0 * d) * vc
    _check(f"rms/{name}/unnorm", "rows", m(v.cuda(), True), u64, tr.bound(floor, s32.unnormalize(v).double() - u64, cols=True))
    torch.cuda.synchronize()
    assert torch.equal(before, m.packed)
