"""KL early stopping decided on the device (kl_early_stop=True: the estimator in column 5 of the loss record, the
decision in the statistics block of k_sumsq_stats, every later kernel of the update gated by the stop word) against the
CPU oracle driven step by step with the reference's breaks live (tests/kl_stop_cases.py).

Every case's margin condition is asserted on the oracle's own sequence before any GPU figure is looked at: steps before
the stop >= 10 % below 1.5 thr, the stop step >= 10 % above.

Per-step estimator against the float64 restatement: rtol 1e-4 + atol A, A = 8 x the largest |fp32 CPU - float64| over
the case's steps (kl_stop_cases.estimator_atol, evaluated where the test runs; the factor covers a device expf one ulp
off libm near 1).  The CPU figure depends on the host's exp and summation order.  Measured on two hosts, per case, as
|fp32 - float64| -> A:  A, B, no_stop, adaptive 6.85e-9 -> 5.5e-8 and 6.04e-9 -> 4.8e-8;  C 2.33e-9 -> 1.9e-8 and
1.16e-9 -> 9.3e-9;  C_contacts 5.08e-9 -> 4.1e-8 and 4.68e-9 -> 3.7e-8;  act8 2.55e-9 -> 2.0e-8 and 1.95e-9 -> 1.6e-8.
The device's largest |estimator - float64| on the MI355X: A, B 8.1e-9, C 9.5e-9 (at a value of 1.0e-2, inside rtol;
4.0e-9 at step 0), C_contacts 6.5e-9, act8 7.1e-9.

What a stopped update leaves is compared bit for bit with an engine built WITHOUT the switch that runs the step-wise
loop for exactly s steps and then the forward / backward half of step s (whose gather publishes step s's running
statistics, and whose loss kernel writes minibatch s's mus / sigmas rows -- the one documented deviation from the
reference, identical in both engines; against the oracle those rows are left out).  The padded / transposed
first-layer copies live in the workspace and are rebuilt by the first gather of every update; they are compared through
what reads them, the policy forward.  Against the oracle: parameters within k * lr * 0.02 (smoke()'s bound) with k = s,
normaliser states rtol 1e-5 with exact counts, the arena outside minibatch s at the free-running bounds of
test_gpu_teacher.py (mus atol 5e-3, sigmas rtol 2e-3), per-step losses rtol 2e-4 / atol 2e-6 (test_gpu_lr_schedule.py)."""
import numpy as np
import pytest
import torch

from tests import kl_stop_cases as K
from tests import lr_schedule_cases as L

pytestmark = pytest.mark.gpu

STATE = ("params", "adam_m", "adam_v", "rms_obs", "rms_priv", "rms_value", "mus_w", "sigmas_w")
STOP_CASES = ["A", "B", "C", "C_contacts", "act8"]


def _engine(name, kl_early_stop=True, thr=None, **kw):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    c = K.CASES[name]
    N, T, E = c["shape"]
    P, Ec = c["contacts"]
    init, ro, perm = K.case_problem(name)
    if c.get("adaptive"):
        kw.setdefault("lr_schedule", "adaptive")
    eng = TeacherEngine(N, T, E, units=c["units"], priv_units=c["priv_units"], perm=perm, obs_dim=L.OBS,
                        act_dim=c.get("act", L.ACT), contact_points=P, contact_emb=Ec, lr=c["lr"],
                        kl_threshold=c["thr"] if thr is None else thr, kl_early_stop=kl_early_stop, **kw)
    eng.load_params(init)
    eng.prepare(ro)
    return eng


def _stepwise_off(name, s, **kw):
    """an engine without the switch: s whole steps, then the forward / backward half of step s"""
    off = _engine(name, kl_early_stop=False, **kw)
    for k in range(s):
        off.fwd_bwd(k % off.n_mb, k)
        off.apply(k)
    off.fwd_bwd(s % off.n_mb, s)
    return off


def _infer(eng, name):
    _, ro, _ = K.case_problem(name)
    n = 32
    args = [ro["obses"][0, :n], ro["priv_info"][0, :n]]
    if K.CASES[name]["contacts"][0]:
        return eng.infer_contacts(*args, ro["contacts"][0, :n])
    return eng.infer(*args)


@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_step_estimator_and_state(name):
    ref = K.case_oracle(name)
    K.assert_margins(name, ref)
    s = ref["stop"]
    eng = _engine(name)
    t0 = eng.adam_t
    eng.update()
    torch.cuda.synchronize()
    got = eng.approx_kl().numpy().astype(np.float64)
    A = K.estimator_atol(ref)
    print(f"{name}: stop {eng.stop_step} (oracle {s}); estimator device {got}, float64 {ref['approx64']}, "
          f"max |diff| {np.abs(got - ref['approx64'][:len(got)]).max():.3e}, atol A {A:.3e}")
    assert eng.stop_step == s and eng.steps_applied == s and eng.adam_t == t0 + s
    assert len(got) == s + 1
    np.testing.assert_allclose(got, ref["approx64"], rtol=1e-4, atol=A, err_msg="approx_kl")
    # ---- bit for bit the switch-off step-wise loop of exactly s steps (+ the forward half of step s)
    off = _stepwise_off(name, s)
    torch.cuda.synchronize()
    assert off.adam_t == t0 + s
    for k in STATE:
        assert torch.equal(getattr(eng, k), getattr(off, k)), k
    assert torch.equal(eng.stats[:s], off.stats[:s])
    for a, b in zip(_infer(eng, name), _infer(off, name)):          # the first-layer copies, through what reads them
        assert torch.equal(a, b)
    # ---- against the oracle
    st = eng.stats.cpu().numpy()
    if name != "B":     # at 3e-3 the clipped losses' kinks flip between the two implementations (test_gpu_lr_schedule.py)
        for j, nm in enumerate(["a_losses", "c_losses", "b_losses"]):
            np.testing.assert_allclose(st[:s, j], ref[nm], rtol=2e-4, atol=2e-6, err_msg=nm)
        # row s: entropy and KL are appended before the break (per-step KL at test_gpu_teacher.py's bound)
        np.testing.assert_allclose(st[:s + 1, 3], ref["entropies"], rtol=2e-4, atol=2e-6, err_msg="entropies")
        np.testing.assert_allclose(st[:s + 1, 4], ref["step_kls"], rtol=1e-2, atol=5e-7, err_msg="per-step KL")
    bound = s * K.CASES[name]["lr"] * 0.02
    pd = np.abs(eng.packed().cpu().numpy() - ref["params"]).max()
    print(f"{name}: parameters max |diff| = {pd:.3e} (bound k lr 0.02 = {bound:.3e})")
    assert pd <= bound
    for packed, key in ((eng.rms_obs, "rms_obs"), (eng.rms_priv, "rms_priv")):
        d = eng.rms_dict(packed)
        mean, var, count = ref[key]
        np.testing.assert_allclose(d["running_mean"].cpu().numpy(), mean, rtol=1e-5, atol=1e-7, err_msg=key)
        np.testing.assert_allclose(d["running_var"].cpu().numpy(), var, rtol=1e-5, err_msg=key)
        assert d["count"].item() == count == 1 + (s + 1) * eng.mb
    keep = np.ones(eng.B, dtype=bool)
    keep[ref["idx_stop"].numpy()] = False                           # minibatch s: the documented deviation
    np.testing.assert_allclose(eng.env_major(eng.mus_w).cpu().numpy()[keep], ref["mus"][keep], atol=5e-3)
    np.testing.assert_allclose(eng.env_major(eng.sigmas_w).cpu().numpy()[keep], ref["sigmas"][keep], rtol=2e-3)


def test_second_update_counts_from_the_stop():
    """adam_t advanced by s: the update that follows uses the bias corrections of s + 1, s + 2, ... -- bit for bit the
    switch-off engine that was stopped by hand, and not what an engine gives that counts all E * n_mb steps"""
    s = K.CASES["C"]["stop"]
    eng = _engine("C")
    eng.update()
    assert eng.adam_t == s
    off, wrong = _stepwise_off("C", s), _stepwise_off("C", s)
    assert off.adam_t == s
    wrong.adam_t = wrong.E * wrong.n_mb
    eng.kl_threshold = 1.0          # nothing stops the second update
    for e in (eng, off, wrong):
        e.prepare()
        e.update()
    torch.cuda.synchronize()
    assert eng.stop_step is None and eng.adam_t == off.adam_t == s + eng.E * eng.n_mb
    for k in STATE + ("stats",):
        assert torch.equal(getattr(eng, k), getattr(off, k)), k
    assert not torch.equal(wrong.params, eng.params)


def test_no_stop_is_the_switch_off_update():
    K.assert_margins("no_stop")
    on, off = _engine("no_stop"), _engine("no_stop", kl_early_stop=False)
    on.update()
    off.update()
    torch.cuda.synchronize()
    assert on.stop_step is None and on.steps_applied == 16 and on.adam_t == off.adam_t == 16
    for k in STATE + ("stats",):
        assert torch.equal(getattr(on, k), getattr(off, k)), k
    ref = K.case_oracle("no_stop")
    got = on.approx_kl().numpy().astype(np.float64)
    print(f"no_stop: estimator device {got}, max |diff| {np.abs(got - ref['approx64']).max():.3e}")
    np.testing.assert_allclose(got, ref["approx64"], rtol=1e-4, atol=K.estimator_atol(ref))


@pytest.mark.parametrize("name", ["C", "A"])
def test_stepwise_loop_equals_the_one_call_update(name):
    free = _engine(name)
    free.update()
    step = _engine(name)
    for k in range(step.E * step.n_mb):
        step.fwd_bwd(k % step.n_mb, k)
        step.apply(k)
    torch.cuda.synchronize()
    s = K.CASES[name]["stop"]
    assert free.stop_step == step.stop_step == s and free.adam_t == step.adam_t == s
    for k in STATE:
        assert torch.equal(getattr(free, k), getattr(step, k)), k
    assert torch.equal(free.stats[:s], step.stats[:s]) and torch.equal(free.stats[s, :5], step.stats[s, :5])
    assert torch.equal(free.approx_kl(), step.approx_kl())


def test_two_runs_are_bit_identical():
    a, b = _engine("A"), _engine("A")
    a.update()
    b.update()
    torch.cuda.synchronize()
    for k in STATE + ("stop_state",):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    s = a.stop_step
    assert torch.equal(a.stats[:s], b.stats[:s]) and torch.equal(a.stats[s, :5], b.stats[s, :5])


def test_adaptive_rate_decides_once_more_on_the_partial_mean():
    ref = K.case_oracle("adaptive")
    K.assert_margins("adaptive", ref)
    s, n_mb = ref["stop"], 4
    eng = _engine("adaptive")
    eng.update()
    torch.cuda.synchronize()
    assert eng.stop_step == s
    hist = eng.lr_history().numpy()
    n = len(ref["lrs"])
    print(f"adaptive: oracle KL {ref['kl_seen']} rates {ref['lrs']}; device record {hist}")
    assert n == s // n_mb + 1
    assert hist[:n, 1].tolist() == ref["lrs"].tolist()             # the partial-mean decision included
    assert eng.lr == ref["lrs"][-1]
    np.testing.assert_allclose(hist[:n, 0], ref["kl_seen"], rtol=5e-3, atol=1e-7)
    # the scheduler never ran again: the record of the mini-epochs behind the stop is untouched
    assert np.all(hist[n:] == 0.0)
    st = eng.stats.cpu().numpy()
    assert np.array_equal(st[:s, 7], ref["step_lr"].astype(np.float32))
    kl_part = st[n_mb * (n - 1):s + 1, 4].astype(np.float32)
    np.testing.assert_allclose(hist[n - 1, 0], np.float64(kl_part.mean(dtype=np.float32)), rtol=1e-6)
    off = _stepwise_off("adaptive", s)                              # the rate schedule alone, stopped by hand
    torch.cuda.synchronize()
    for k in ("params", "adam_m", "adam_v", "rms_obs", "rms_priv"):
        assert torch.equal(getattr(eng, k), getattr(off, k)), k


def _launches(fn):
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for c in _lib.prof_read():
            key = c["name"].split(":")[0].split("#")[0]
            out[key] = out.get(key, 0) + c["launches"]
    finally:
        _lib.prof_enable(False)
    return out


@pytest.mark.parametrize("name, loss", [("A", "k_trunk_loss"), ("B", "k_trunk_loss")])
def test_host_stops_enqueueing_one_mini_epoch_behind_the_stop(name, loss):
    """a stop in mini-epoch e: mini-epochs 0 .. e + 1 are enqueued, nothing beyond (the three-mini-epoch cases have
    nothing beyond e + 1 to save)"""
    eng = _engine(name)
    runs = _launches(eng.update)
    s, n_mb, E = K.CASES[name]["stop"], eng.n_mb, eng.E
    assert eng.stop_step == s
    want = min(s // n_mb + 2, E) * n_mb
    print(f"{name}: stop {s} in mini-epoch {s // n_mb}: {runs.get(loss)} loss launches of {E * n_mb}")
    assert want < E * n_mb and runs[loss] == runs["k_sumsq_stats"] == want
    off = _engine(name, kl_early_stop=False)
    assert _launches(off.update)[loss] == E * n_mb


def test_trainer_slices_its_lists(tmp_path):
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=64, horizon_length=8, rl_device="cuda:0", mini_epochs=4, num_points=8,
                         kl_early_stop=True, kl_threshold=1.0)
    cfg.train.network.mlp.units = [64, 48, 32]
    cfg.train.network.priv_mlp.units = [48, 32, 8]
    env = SyntheticInsertionEnv(num_envs=64, device="cuda:0")
    agent = PPO(env, str(tmp_path), cfg)
    eng = agent.engine
    assert eng.kl_early_stop and agent.kl_early_stop
    lr0 = agent.last_lr
    agent.obs = env.reset()
    out = agent.train_epoch()                       # threshold 1: runs through
    E, n_mb = eng.E, eng.n_mb
    assert [len(x) for x in out[:6]] == [E * n_mb] * 4 + [E] + [E * n_mb]
    assert eng.stop_step is None and agent.extra_info["info/opt_steps"] == E * n_mb
    assert agent.optimizer.state_dict()["step"] == E * n_mb
    first = eng.approx_kl().numpy()
    assert agent.extra_info["info/approx_kl"] == float(first[-1])
    # a threshold the next update crosses part of the way: 1.5 thr = the geometric mean of this update's steps 1 and 2
    eng.kl_threshold = float(np.sqrt(first[1] * first[2])) / 1.5
    out = agent.train_epoch()
    s = eng.stop_step
    print(f"trainer: first update's estimator {first}, second update stopped at {s}: {eng.approx_kl().numpy()}")
    assert s is not None and 0 < s < E * n_mb
    e = s // n_mb
    assert [len(x) for x in out[:6]] == [s, s, s, s + 1, e + 1, s]
    st = eng.stats
    assert torch.equal(torch.stack(out[0]), st[:s, 0]) and torch.equal(torch.stack(out[3]), st[:s + 1, 3])
    assert out[4][-1] == st[e * n_mb:s + 1, 4].mean()
    assert agent.extra_info["info/opt_steps"] == s and agent.extra_info["info/approx_kl"] == float(eng.approx_kl()[-1])
    assert agent.optimizer.state_dict()["step"] == eng.adam_t == E * n_mb + s
    assert agent.last_lr == lr0 == agent.optimizer.param_groups[0]["lr"]


def test_refusals():
    from isaacgyminsertion_amd import ops
    eng = _engine("C")
    with pytest.raises(RuntimeError, match="two-phase"):
        eng.fwd_bwd_phase(0, 0, 0)
    st, icfg, fcfg = eng._stop_args()
    assert len(st) == 17 and st[-1] is eng.stop_state and icfg[-1] == 1 and fcfg[-1] == eng.kl_threshold
    with pytest.raises(RuntimeError, match="stop_state"):              # a stop tensor of the wrong length
        torch.ops.mi355ppo.ppo_update(eng._ro, st[:-1] + [eng.stop_state[:-1].contiguous()], icfg, fcfg, 0)
    with pytest.raises(RuntimeError):                                   # the tail's int and float without its tensor
        torch.ops.mi355ppo.ppo_update(eng._ro, st[:-1], icfg, fcfg, 0)
    with pytest.raises(RuntimeError, match="phase"):
        torch.ops.mi355ppo.ppo_minibatch_fwd_bwd(eng._ro, st, icfg, fcfg, 0, 0, 0)
    # the other ops keep today's lists
    assert len(eng.state_list()) == 16 and len(eng._cfg_args()[1]) == 12 and len(ops.STATE_FIELDS) == 16
    with pytest.raises(ValueError):
        _engine("C", thr=0.0)


def test_cpp_and_python_registrations_agree(tmp_path):
    """The C++ registration (csrc/torch_ops.cpp) takes the same early-stopping tail as ops.py and gives the same bits;
    hand-built lists of today's length keep meaning "off" (tests/cpp_ops_stop_child.py, one registration per process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "isaacgyminsertion_amd", "libigi_torch_ops.so")):
        pytest.skip("libigi_torch_ops.so not built on this host (python -c 'import __graft_entry__ as g; g.build()')")
    got = {}
    for which in ("cpp", "py"):
        path = str(tmp_path / f"{which}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "cpp_ops_stop_child.py"), which, path], cwd=root,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (which, r.stdout[-2000:], r.stderr[-3000:])
        got[which] = np.load(path)
    A, B = got["cpp"], got["py"]
    assert set(A.files) == set(B.files)
    for k in A.files:
        assert A[k].shape == B[k].shape and np.array_equal(A[k], B[k]), k
    assert A["refused"].tolist() == [1, 1, 1, 1, 1]
    # a threshold nothing reaches: the bits of today's lists
    assert A["stop_through"][0] == -1
    assert np.array_equal(A["params_through"], A["params_plain"]) and np.array_equal(A["stats_through"], A["stats_plain"])
    # 1.5 thr between the recorded estimator of step k and the largest before it: the same run stops at k, in one call
    # and step by step
    seq = A["stop_through"][2:].view(np.float32)
    limit, k = 1.5 * float(A["thr"]), int(A["target"])
    print(f"registrations: estimator {seq}, 1.5 thr {limit:.4e}, stop aimed at {k}, got {A['stop_stopped'][0]}")
    assert k >= 3 and seq[:k].max() < limit < seq[k]
    assert A["stop_stopped"][0] == A["stop_stepwise"][0] == k
    assert np.array_equal(A["stop_stopped"][2:3 + k], A["stop_through"][2:3 + k])
    assert np.array_equal(A["params_stopped"], A["params_stepwise"])
    assert not np.array_equal(A["params_stopped"], A["params_through"])


def test_one_threshold_for_the_stop_and_the_scheduler():
    """under lr_schedule adaptive the engine's kl_threshold is the cfg's; lists that disagree are refused"""
    eng = _engine("adaptive")
    assert eng.kl_threshold == eng.cfg.kl_threshold == K.CASES["adaptive"]["thr"]
    eng.kl_threshold = 2e-3
    assert eng.cfg.kl_threshold == 2e-3
    st, icfg, fcfg = eng._stop_args()
    assert fcfg[12] == fcfg[-1] == 2e-3 and len(fcfg) == 16
    with pytest.raises(RuntimeError, match="differs"):
        torch.ops.mi355ppo.ppo_update(eng._ro, st, icfg, fcfg[:-1] + [3e-3], 0)
    with pytest.raises(ValueError):
        eng.kl_threshold = 0.0


def test_one_read_of_the_stop_record_per_update():
    eng = _engine("C")
    eng.update()
    assert eng._stop_words is None
    s = eng.stop_step
    rec = eng._stop_words
    assert rec is not None and not rec.is_cuda
    assert eng.steps_applied == s and eng.adam_t == s and len(eng.approx_kl()) == s + 1
    assert eng._stop_words is rec                      # the four figures came from the one copy
    eng.prepare()
    eng.update()
    assert eng._stop_words is None                     # a new update drops it
