"""The KL-adaptive learning rate scheduled on the device (lr_schedule="adaptive": csrc/teacher.h k_lr_schedule, the
rate read by both Adam tails from igi_teacher_state.lr_state) against the CPU oracle driven one mini-epoch at a time with
AdaptiveScheduler.update in between (tests/lr_schedule_cases.py) -- the reference's loop with frozen_ppo.py:630 live.

Bounds, none of them new: the rate record equals the oracle's double sequence EXACTLY (the device restates the Python
doubles; every oracle KL is >= 10 % away from both decision boundaries, 20 x the KL tolerance); stats slot 7 ==
float32(rate of the step's mini-epoch); per-epoch KL rtol 5e-3 / atol 1e-7 (test_gpu_teacher.py); per-step losses rtol
2e-4 / atol 2e-6 and final parameters within 0.05 * sum of the per-step rates (test_gpu_teacher_shapes.py's steps * lr *
0.05 with the rate no longer constant).

Under the FIXED schedule stats slot 7 keeps what it has always held in the teacher's rows, the clip coefficient
min(grad_norm / (total_norm + 1e-6), 1) (include/igi_ppo.h used to document the slot as 0; the kernel never wrote 0
there): fixed is today's behaviour bit for bit, which test_fixed_schedule_is_untouched pins from slot 5."""
import numpy as np
import pytest
import torch

from tests import lr_schedule_cases as L

pytestmark = pytest.mark.gpu

SCHED = "k_lr_schedule"


def _engine(name, lr_schedule="adaptive", **kw):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    (N, T, E), units, priv_units, lr0, thr, (P, Ec) = L.CASES[name]
    init, ro, perm = L.case_problem(name)
    eng = TeacherEngine(N, T, E, units=units, priv_units=priv_units, perm=perm, obs_dim=L.OBS, contact_points=P,
                        contact_emb=Ec, lr=lr0, lr_schedule=lr_schedule, kl_threshold=thr, **kw)
    eng.load_params(init)
    eng.prepare(ro)
    return eng


def _epoch_kl(eng):
    return eng.stats.cpu().numpy()[:, 4].reshape(eng.E, eng.n_mb).mean(1)


def _check_record(name, eng, ref):
    """rate record == oracle doubles, slot 7 == float32(rate of the step), per-epoch KL at test_gpu_teacher's bound"""
    lr0 = L.CASES[name][3]
    L.assert_margins(ref)
    hist = eng.lr_history().numpy()
    kl = _epoch_kl(eng)
    print(f"{name}: oracle KL {ref['kls'][0]}, device KL {hist[:, 0]}, rates {hist[:, 1]}, "
          f"decisions {L.decisions(lr0, hist[:, 1])}")
    np.testing.assert_allclose(kl, ref["kls"][0], rtol=5e-3, atol=1e-7, err_msg="per-epoch KL")
    # the KL the scheduler compared is the fp32 mean of the mini-epoch's slot-4 values (last-bit room for the order of
    # the fp32 sum against numpy's)
    np.testing.assert_allclose(hist[:, 0], kl.astype(np.float64), rtol=1e-6)
    assert hist[:, 1].tolist() == ref["lrs"][0].tolist(), (hist[:, 1], ref["lrs"][0])
    assert eng.lr == ref["lrs"][0][-1]
    assert L.decisions(lr0, hist[:, 1]) == L.EXPECTED[name]
    slot7 = eng.stats.cpu().numpy()[:, 7]
    assert np.array_equal(slot7, ref["step_lr"][0].astype(np.float32)), (slot7, ref["step_lr"][0])


def _state(eng):
    return {k: getattr(eng, k).clone() for k in ("params", "adam_m", "adam_v", "stats", "lr_state", "rms_obs", "rms_priv",
                                                 "mus_w", "sigmas_w")}


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_free_running_update_matches_the_scheduled_oracle(name):
    ref = L.case_oracle(name)
    eng = _engine(name)
    eng.update()
    torch.cuda.synchronize()
    _check_record(name, eng, ref)
    s = eng.stats.cpu().numpy()
    if name == "B":
        # at 3e-3 the clipped losses' kinks flip between the two implementations: no parameter bound; the run is
        # deterministic instead
        other = _engine(name)
        other.update()
        torch.cuda.synchronize()
        for k, v in _state(eng).items():
            assert torch.equal(v, getattr(other, k)), k
        return
    for j, nm in enumerate(["a_losses", "c_losses", "b_losses", "entropies"]):
        np.testing.assert_allclose(s[:, j], ref[nm][0], rtol=2e-4, atol=2e-6, err_msg=nm)
    bound = 0.05 * ref["step_lr"][0].sum()
    pd = np.abs(eng.packed().cpu().numpy() - ref["params"]).max()
    print(f"{name}: final parameters max |diff| = {pd:.3e} (bound {bound:.3e})")
    assert pd <= bound


def test_stepwise_loop_equals_update_bit_for_bit():
    """fwd_bwd + apply under the schedule (the scheduler runs inside apply when the slot ends a mini-epoch)"""
    free = _engine("C")
    free.update()
    step = _engine("C")
    slot = 0
    for _ in range(step.E):
        for i in range(step.n_mb):
            step.fwd_bwd(i, slot)
            step.apply(slot)
            slot += 1
    torch.cuda.synchronize()
    assert step.adam_t == free.adam_t == slot
    a, b = _state(free), _state(step)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert L.decisions(1e-3, free.lr_history()[:, 1].tolist()) == L.EXPECTED["C"]


def test_rate_carries_over_and_tune_workspace_restores_it():
    from isaacgyminsertion_amd import ops
    ref = L.case_oracle("A")
    eng = _engine("A")
    eng.update()
    torch.cuda.synchronize()
    first = eng.lr_history().numpy()
    assert first[:, 1].tolist() == ref["lrs"][0].tolist()
    keys = [k for k in ops.STATE_FIELDS if k != "workspace"] + ["lr_state"]
    before = {k: getattr(eng, k).clone() for k in keys}
    t0 = eng.adam_t
    times = eng.tune_workspace(trials=3)
    torch.cuda.synchronize()
    assert times is not None and len(times) == 3
    assert eng.adam_t == t0
    for k in keys:
        assert torch.equal(before[k], getattr(eng, k)), k
    eng.prepare()
    eng.update()
    torch.cuda.synchronize()
    second = eng.lr_history().numpy()
    s7 = eng.stats.cpu().numpy()[:, 7]
    assert s7[0] == np.float32(first[-1, 1])                  # the second update starts at the first's final rate
    prev = first[-1, 1]
    for e in range(eng.E):                                     # and its record is the rule applied to its own KL
        assert np.all(s7[e * eng.n_mb:(e + 1) * eng.n_mb] == np.float32(prev))
        prev = L.rule(prev, second[e, 0], L.CASES["A"][4])
        assert second[e, 1] == prev
    assert eng.lr == prev


@pytest.mark.parametrize("name, clamp, value", [("A", "lr_max", 3e-4), ("B", "lr_min", 2.5e-3)])
def test_clamps(name, clamp, value):
    ref = L.case_oracle(name, **{clamp: value})
    L.assert_margins(ref)
    assert ref["lrs"][0].tolist() == [value] * 4              # the first move hits the clamp, later ones stay on it
    eng = _engine(name, **{clamp: value})
    eng.update()
    torch.cuda.synchronize()
    hist = eng.lr_history().numpy()
    print(f"{name} {clamp}={value}: oracle KL {ref['kls'][0]}, device KL {hist[:, 0]}, rates {hist[:, 1]}")
    lr = L.CASES[name][3]
    for e in range(eng.E):                                     # the record is the clamped rule on the KL it compared
        lr = L.rule(lr, hist[e, 0], L.CASES[name][4], **{clamp: value})
        assert hist[e, 1] == lr
    assert hist[:, 1].tolist() == [value] * 4
    s7 = eng.stats.cpu().numpy()[:, 7]
    assert np.all(s7[:eng.n_mb] == np.float32(L.CASES[name][3])) and np.all(s7[eng.n_mb:] == np.float32(value))


def test_contacts_share_the_scheduled_tail():
    """C's shape with ground-truth contacts (P = 37, E = 8): rate sequence and KL only"""
    ref = L.case_oracle("C_contacts")
    eng = _engine("C_contacts")
    eng.update()
    torch.cuda.synchronize()
    _check_record("C_contacts", eng, ref)


def _launches(fn):
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for c in _lib.prof_read():
            out[c["name"]] = out.get(c["name"], 0) + c["launches"]
    finally:
        _lib.prof_enable(False)
    return out


def test_fixed_schedule_is_untouched():
    from isaacgyminsertion_amd import _lib, ops
    M = _lib.IGI_MAX_LAYERS
    fixed = _engine("A", lr_schedule="fixed")
    icfg, fcfg = fixed._cfg_args()
    assert (len(icfg), len(fcfg), len(fixed.state_list())) == (8 + 2 * M, 12, 16) and len(ops.STATE_FIELDS) == 16
    assert fixed.lr_state is None and fixed.lr == 2.5e-4
    runs = _launches(fixed.update)
    assert runs.get(SCHED, 0) == 0 and runs["k_adam_gather"] == 15 and runs["k_clip_adam"] == 1
    s = fixed.stats.cpu().numpy()
    # slot 7 is what the fixed path has always written there: the clip coefficient of the step, never a rate
    coef = np.minimum(np.float32(1.0) / (s[:, 5] + np.float32(1e-6)), np.float32(1.0)).astype(np.float32)
    assert np.array_equal(s[:, 7], coef)
    # bit for bit the engine built without the new arguments
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    (N, T, E), units, priv_units, lr0, thr, _ = L.CASES["A"]
    init, ro, perm = L.case_problem("A")
    plain = TeacherEngine(N, T, E, units=units, priv_units=priv_units, perm=perm, obs_dim=L.OBS, lr=lr0)
    plain.load_params(init)
    plain.prepare(ro)
    assert plain._cfg_args() == (icfg, fcfg)
    plain.update()
    torch.cuda.synchronize()
    for k in ("params", "adam_m", "adam_v", "stats"):
        assert torch.equal(getattr(plain, k), getattr(fixed, k)), k
    # under the schedule: exactly E scheduler launches per update, the appended fields and the extra state tensor
    ada = _engine("A")
    icfg2, fcfg2 = ada._cfg_args()
    assert icfg2 == icfg + [1] and fcfg2 == fcfg + [thr, 1e-6, 1e-2] and len(ada.state_list()) == 17
    runs = _launches(ada.update)
    assert runs[SCHED] == E and runs["k_adam_gather"] == 15 and runs["k_clip_adam"] == 1


def test_trainer_follows_the_device_rate(tmp_path):
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=64, horizon_length=8, rl_device="cuda:0", mini_epochs=4, num_points=8,
                         lr_schedule="adaptive")
    cfg.train.network.mlp.units = [64, 48, 32]
    cfg.train.network.priv_mlp.units = [48, 32, 8]
    env = SyntheticInsertionEnv(num_envs=64, device="cuda:0")
    agent = PPO(env, str(tmp_path), cfg)
    lr0 = float(cfg.train.ppo.learning_rate)
    assert agent.engine.adaptive_lr and agent.last_lr == lr0
    agent.obs = env.reset()
    agent.train_epoch()
    s7 = agent.engine.stats.cpu().numpy()[:, 7]
    assert s7[0] == np.float32(lr0)
    rate = agent.last_lr
    assert rate != lr0                                           # moved from the configured rate
    assert rate == agent.optimizer.param_groups[0]["lr"] == agent.optimizer.state_dict()["lr"] == agent.engine.lr
    assert rate == agent.engine.lr_history()[-1, 1].item()
    agent.optimizer.param_groups[0]["lr"] = 7e-4                 # a rate set by hand is the one the next step uses
    agent.train_epoch()
    s7 = agent.engine.stats.cpu().numpy()[:, 7]
    assert s7[0] == np.float32(7e-4)
    assert agent.last_lr == agent.optimizer.param_groups[0]["lr"] == agent.optimizer.state_dict()["lr"] == agent.engine.lr
    assert agent.last_lr == agent.engine.lr_history()[-1, 1].item()
    # a checkpointed optimizer puts its rate back on the device
    sd = dict(agent.optimizer.state_dict(), lr=3e-4)
    agent.optimizer.load_state_dict(sd)
    assert agent.engine.lr == 3e-4 and agent.optimizer.param_groups[0]["lr"] == 3e-4


def test_cpp_and_python_registrations_agree_under_the_schedule(tmp_path):
    """The C++ registration (csrc/torch_ops.cpp) takes the same longer lists as ops.py and gives the same bits; both
    refuse a list that is short of the schedule's tensor, int or floats (tests/cpp_ops_lr_child.py, one registration per
    process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "isaacgyminsertion_amd", "libigi_torch_ops.so")):
        pytest.skip("libigi_torch_ops.so not built on this host (python -c 'import __graft_entry__ as g; g.build()')")
    got = {}
    for which in ("cpp", "py"):
        path = str(tmp_path / f"{which}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "cpp_ops_lr_child.py"), which, path], cwd=root,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (which, r.stdout[-2000:], r.stderr[-3000:])
        got[which] = np.load(path)
    A, B = got["cpp"], got["py"]
    assert set(A.files) == set(B.files)
    for k in A.files:
        assert A[k].shape == B[k].shape and np.array_equal(A[k], B[k]), k
    assert A["refused"].tolist() == [1, 1, 1, 1]
    rec = A["lr_state"][2:].reshape(4, 2)
    lr = 2.5e-4
    for e in range(4):                      # threshold 0.004: the record is the rule on the KL it compared
        assert np.all(A["stats"][4 * e:4 * e + 4, 7] == np.float32(lr))
        lr = L.rule(lr, rec[e, 0], 0.004)
        assert rec[e, 1] == lr
    assert lr != 2.5e-4 and A["lr_state2"][0] != A["lr_state"][0] and np.isfinite(A["params_after2"]).all()
