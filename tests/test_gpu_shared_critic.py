"""Teacher PPO with a shared actor-critic trunk (train.ppo.shared_parameters) on the device: whole updates against goldens
captured from the REFERENCE's own PPO (tests/golden/make_golden_teacher_shared.py) and against the shared restatement
(tests/shared_critic_ref.py, pinned to those goldens on the CPU), inference and the rollout policy step against
float64, the bit-level properties of the update drivers, and the trainers.

Tolerances: against the goldens test_contact_teacher_matches_reference_golden's (tests/test_gpu_teacher_contacts_golden.py:
returns_raw bit-equal, advantages 2e-5 + 1e-5 relative, step-0 gradient 1e-4 of the largest entry + 1e-3 relative, loss
columns 1e-4 relative + 1e-6, mini-epoch KL 2e-3 relative, gradient norm 1e-3, parameter norm 1e-5, final parameters
steps * lr * 0.02 per update, scattered mus 2e-4; the normaliser states, which that test does not look at, at
test_teacher_matches_reference_golden's of tests/test_gpu_teacher.py: value statistics after prepare 1e-6, running means
1e-5 + 1e-7, running variances 1e-5 -- fp32 batch moments merged in fp64 -- and the counts equal); against the restatement test_ragged_configs_match_oracle's, as quoted in
tests/test_gpu_teacher_shapes.py (returns_raw bit-equal, advantages 5e-5, step-0 gradient 2e-4 of the largest entry +
2e-3 relative, loss columns 2e-4 relative + 2e-6, final parameters steps * lr * 0.05, scattered mus 2e-5).  Where a
branch is a launch the profiler sees, its class is asserted (csrc/prof.h), as in that file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import shared_critic_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIV = 64
DEFAULT_UNITS, DEFAULT_PRIV_UNITS = [512, 256, 128], [256, 128, 8]
SMALL_UNITS, SMALL_PRIV_UNITS = [64, 48, 32], [48, 32, 8]
K_LATB, K_FWD12 = "k_latent_bwd", "k_fwd12"
K_RB_TRUNK, K_RB_ENV, K_TRUNK_LOSS, K_LOSS = "k_rb_level#trunk3", "k_rb_level#env2", "k_trunk_loss", "k_loss"
KEYS = ("obses", "priv_info", "rewards", "values", "neglogpacs", "dones", "actions", "mus", "sigmas", "last_values")


def _engine(N, T, Ep, units, priv_units, init, perm, obs_dim=15, act_dim=6, shared=True, **kw):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    if shared is not None:
        kw["shared_parameters"] = shared
    eng = TeacherEngine(N, T, Ep, units=units, priv_units=priv_units, perm=perm, obs_dim=obs_dim, act_dim=act_dim, **kw)
    eng.load_params(init)
    return eng


def _step0_classes(eng):
    """fwd_bwd(0, 0) under the library's profiler: {class: launches}."""
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        eng.fwd_bwd(0, 0)
        torch.cuda.synchronize()
        classes = {}
        for c in _lib.prof_read():
            name = c["name"].split(":")[0]
            classes[name] = classes.get(name, 0) + c["launches"]
    finally:
        _lib.prof_enable(False)
    print("launches of step 0:", {k: v for k, v in sorted(classes.items()) if v})
    return classes


def _assert_classes(classes, kernels, absent=()):
    for name, count in (kernels or {}).items():
        assert classes.get(name, 0) == count, (name, count, classes)
    for name in absent:
        assert not any(k.startswith(name) and v for k, v in classes.items()), (name, classes)


# ---- 1. the reference's own numbers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "default"])
def test_shared_teacher_matches_reference_golden(case):
    g, meta, init = sr.load(case)
    eng = _engine(meta["num_envs"], meta["horizon"], meta["mini_epochs"], meta["units"], meta["priv_units"], init,
                  torch.from_numpy(g["perm"]))
    assert eng.shared_parameters and len(eng.shapes) == 17
    lr = 2.5e-4
    for u in range(meta["n_updates"]):
        ro = {k: torch.from_numpy(g[f"u{u}/in/{k}"]).cuda() for k in KEYS}
        eng.prepare(ro)
        torch.cuda.synchronize()
        assert np.array_equal(eng.returns_raw.cpu().numpy(), g[f"u{u}/returns_raw"])
        np.testing.assert_allclose(eng.env_major(eng.advantages).cpu().numpy(), g[f"u{u}/advantages"], atol=2e-5,
                                   rtol=1e-5)
        np.testing.assert_allclose(eng.rms_value.cpu().numpy(), g[f"u{u}/vms_after_tail"], rtol=1e-6)
        eng.fwd_bwd(0, 0)
        torch.cuda.synchronize()
        g0 = eng.packed(eng.grads).cpu().numpy()
        ref0 = g[f"u{u}/grad_step0"]
        print(f"u{u} step-0 gradient: max |diff| / max |ref| = {np.abs(g0 - ref0).max() / np.abs(ref0).max():.3e}")
        np.testing.assert_allclose(g0, ref0, atol=1e-4 * np.abs(ref0).max(), rtol=1e-3)
        eng.apply(0)
        slot = 1
        n_steps = meta["mini_epochs"] * eng.n_mb
        for e in range(meta["mini_epochs"]):
            for i in range(eng.n_mb):
                if e == 0 and i == 0:
                    continue
                eng.fwd_bwd(i, slot)
                eng.apply(slot)
                slot += 1
        torch.cuda.synchronize()
        s = eng.stats.cpu().numpy()
        for j, nm in enumerate(["a_losses", "c_losses", "b_losses", "entropies"]):
            np.testing.assert_allclose(s[:n_steps, j], g[f"u{u}/{nm}"][:n_steps], rtol=1e-4, atol=1e-6, err_msg=nm)
        kls = s[:, 4].reshape(meta["mini_epochs"], eng.n_mb).mean(1)
        np.testing.assert_allclose(kls, g[f"u{u}/kls"], rtol=2e-3, atol=1e-7)
        np.testing.assert_allclose(s[:, 5], g[f"u{u}/grad_total_norms"], rtol=1e-3)
        np.testing.assert_allclose(s[:, 6], g[f"u{u}/param_norms"], rtol=1e-5)
        pd = np.abs(eng.packed().cpu().numpy() - g[f"u{u}/params_after"]).max()
        print(f"u{u} final parameters: max |diff| = {pd:.3e} (bound {n_steps * lr * 0.02 * (u + 1):.3e})")
        np.testing.assert_allclose(eng.packed().cpu().numpy(), g[f"u{u}/params_after"],
                                   atol=n_steps * lr * 0.02 * (u + 1), rtol=0)
        np.testing.assert_allclose(eng.env_major(eng.mus_w).cpu().numpy(), g[f"u{u}/mus_after"], atol=2e-4)
        np.testing.assert_allclose(eng.env_major(eng.sigmas_w).cpu().numpy(), g[f"u{u}/sigmas_after"], rtol=1e-6)
        for nm, st in (("running_mean_std", eng.rms_obs), ("priv_mean_std", eng.rms_priv), ("value_mean_std", eng.rms_value)):
            d = eng.rms_dict(st.cpu())
            np.testing.assert_allclose(d["running_mean"].numpy(), g[f"u{u}/{nm}/running_mean"], rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(d["running_var"].numpy(), g[f"u{u}/{nm}/running_var"], rtol=1e-5)
            assert d["count"].item() == g[f"u{u}/{nm}/count"].item()


# ---- 2 - 5. the restatement, branch by branch ------------------------------------------------------------------------
def _update_vs_restatement(N, T, Ep, units, priv_units, obs_dim=15, act_dim=6, max_steps=None, kernels=None, absent=(),
                           seed=1234):
    """prepare, the step-0 gradient, then EVERY optimizer step of one update (or max_steps of them) with fwd_bwd + apply
    (tests/test_gpu_teacher_shapes.py's _update_vs_oracle on the shared restatement)."""
    init, ro, perm = sr.problem(N, T, units, priv_units, obs_dim=obs_dim, act_dim=act_dim, seed=seed)
    eng = _engine(N, T, Ep, units, priv_units, init, perm, obs_dim, act_dim)
    orc = sr.SharedTeacherOracle(init, perm, N, T, Ep, units, priv_units, obs_dim=obs_dim, act_dim=act_dim)
    d = orc.prepare(ro)
    eng.prepare(ro)
    torch.cuda.synchronize()
    assert torch.equal(eng.returns_raw.cpu(), orc.returns_raw)
    np.testing.assert_allclose(eng.env_major(eng.advantages).cpu().numpy(), d["advantages"].numpy(), atol=5e-5)
    st = orc.update(record_grads=1, max_steps=max_steps)
    _assert_classes(_step0_classes(eng), kernels, absent)
    ref = st["grads"][0].numpy()
    got = eng.packed(eng.grads).cpu().numpy()
    gmax = np.abs(ref).max()
    print(f"step-0 gradient: max |diff| / max |ref| = {np.abs(got - ref).max() / gmax:.3e}")
    np.testing.assert_allclose(got, ref, atol=2e-4 * gmax, rtol=2e-3)
    gv = {k: v.cpu().numpy() for k, v in eng.param_views(eng.grads).items()}
    off = 0
    for k, v in init.items():                       # the two heads and sigma on their own scale
        r = ref[off:off + v.numel()].reshape(v.shape)
        off += v.numel()
        if k in ("value.weight", "value.bias", "mu.weight", "mu.bias", "sigma") and np.abs(r).max() > 0:
            np.testing.assert_allclose(gv[k], r, atol=2e-4 * np.abs(r).max(), rtol=2e-3, err_msg=k)
    eng.apply(0)
    slot = 1
    total = Ep * eng.n_mb if max_steps is None else max_steps
    for e in range(Ep):
        for i in range(eng.n_mb):
            if (e == 0 and i == 0) or slot >= total:
                continue
            eng.fwd_bwd(i, slot)
            eng.apply(slot)
            slot += 1
    torch.cuda.synchronize()
    assert slot == total == len(st["a_losses"])
    s = eng.stats.cpu().numpy()
    for j, nm in enumerate(["a_losses", "c_losses", "b_losses", "entropies"]):
        np.testing.assert_allclose(s[:slot, j], np.array([x.item() for x in st[nm]]), rtol=2e-4, atol=2e-6, err_msg=nm)
    pd = np.abs(eng.packed().cpu().numpy() - orc.flat_params().numpy()).max()
    print(f"final parameters after {slot} steps: max |diff| = {pd:.3e} (bound {slot * 2.5e-4 * 0.05:.3e})")
    np.testing.assert_allclose(eng.packed().cpu().numpy(), orc.flat_params().numpy(), atol=slot * 2.5e-4 * 0.05)
    rows = perm[:eng.mb * min(slot, eng.n_mb)].numpy() if max_steps is not None else slice(None)
    np.testing.assert_allclose(eng.env_major(eng.mus_w).cpu().numpy()[rows], orc.data["mus"].detach().numpy()[rows],
                               atol=2e-5)
    return eng


FUSED = {K_TRUNK_LOSS: 1, K_LOSS: 0}
TRUNK_LOSS_CASES = {
    # name: (N, T, Ep), act           default widths: the shared mode of k_trunk_loss, ONE launch, k_loss never
    "mb64": ((16, 8, 2), 6),          # one 64-row tile
    "mb200": ((50, 8, 2), 6),         # three tiles and eight ragged rows
    "act1": ((50, 8, 2), 1),          # 2 head columns
    "act7": ((50, 8, 2), 7),          # 8 head columns: the whole [64][8] image
}


@pytest.mark.parametrize("case", list(TRUNK_LOSS_CASES))
def test_fused_trunk_loss_in_shared_mode(case):
    (N, T, Ep), act = TRUNK_LOSS_CASES[case]
    _update_vs_restatement(N, T, Ep, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, act_dim=act, kernels=FUSED)


def test_row_block_trunk_level_with_one_net():
    """mb = 256, default widths: trunk layer 2's backward level is the row-block kernel, launched once, on ONE net."""
    from isaacgyminsertion_amd import _lib
    assert _lib.lib().igi_level_backward_parts(256, 256, 1) > 0
    _update_vs_restatement(64, 8, 2, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, kernels=dict(FUSED, **{K_RB_TRUNK: 1, K_LATB: 1}))


def test_update_at_the_fused_forward_row_threshold():
    """mb = 2048 reaches k_fwd12's row threshold: a shared trunk declines that kernel (it runs two nets' first layer), the
    per-layer launches run, and the step matches all the same."""
    _update_vs_restatement(256, 16, 2, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, max_steps=1,
                           kernels=dict(FUSED, **{K_RB_TRUNK: 1, K_RB_ENV: 1, K_LATB: 1}), absent=(K_FWD12,))


SMALL = (100, 6, 3)      # mb = 200; 9 optimizer steps
OTHER_CASES = {
    # name: (N, T, Ep), units, priv_units, obs_dim, act, {class: launches in step 0}
    "one_trunk_layer_128": (SMALL, [128], [24, 16, 8], 15, 6, {K_TRUNK_LOSS: 0, K_LOSS: 1, K_LATB: 1}),   # layer 0 is the last layer
    "last_layer_48": (SMALL, [64, 48], [24, 16, 8], 15, 6, {K_TRUNK_LOSS: 0, K_LOSS: 1, K_LATB: 1}),
    "act8": (SMALL, [64, 48, 32], [24, 16, 8], 15, 8, {K_TRUNK_LOSS: 0, K_LOSS: 1}),                     # k_loss proper (act == 8)
    "four_layers": (SMALL, [96, 64, 48, 32], [48, 32, 16, 8], 15, 6, {K_TRUNK_LOSS: 0, K_LOSS: 1, K_LATB: 1}),
    "latent5": (SMALL, [48, 40, 24], [24, 16, 5], 15, 6, {K_LATB: 0}),                                   # the generic latent data gradient, K = u0
    "latent12": (SMALL, [48, 40, 24], [32, 16, 12], 15, 6, {K_LATB: 0}),
    "xw33": (SMALL, [48, 40, 24], [24, 16, 8], 25, 6, {K_LATB: 1}),                                      # obs + latent = 33: xld = 64
}


@pytest.mark.parametrize("case", list(OTHER_CASES))
def test_shared_update_off_the_default_widths(case):
    (N, T, Ep), units, priv_units, obs_dim, act, kernels = OTHER_CASES[case]
    _update_vs_restatement(N, T, Ep, units, priv_units, obs_dim=obs_dim, act_dim=act, kernels=kernels)


# ---- 6. inference and the rollout policy step --------------------------------------------------------------------------
INFER_CASES = {"default": (DEFAULT_UNITS, DEFAULT_PRIV_UNITS, 15), "off_default": ([48, 40, 24], [32, 16, 12], 15),
               "xw33": ([48, 40, 24], [24, 16, 8], 25)}


def _infer_setup(case, rows):
    units, priv_units, obs_dim = INFER_CASES[case]
    N, T, Ep = 64, 8, 2
    init, ro, perm = sr.problem(N, T, units, priv_units, obs_dim=obs_dim, seed=77)
    g = torch.Generator().manual_seed(1000 + len(case) + rows)
    init["sigma"] = 0.3 * torch.randn(6, generator=g)
    init["value.bias"] = 0.2 * torch.randn(1, generator=g)
    init["mu.bias"] = 0.2 * torch.randn(6, generator=g)
    eng = _engine(N, T, Ep, units, priv_units, init, perm, obs_dim)
    mean_o, var_o = 0.3 * torch.randn(obs_dim, generator=g).double(), (0.5 + torch.rand(obs_dim, generator=g)).double()
    mean_p, var_p = 0.3 * torch.randn(PRIV, generator=g).double(), (0.5 + torch.rand(PRIV, generator=g)).double()
    eng.rms_obs[:obs_dim], eng.rms_obs[obs_dim:2 * obs_dim] = mean_o.cuda(), var_o.cuda()
    eng.rms_priv[:PRIV], eng.rms_priv[PRIV:2 * PRIV] = mean_p.cuda(), var_p.cuda()
    obs = 1.5 * torch.randn(rows, obs_dim, generator=g) + 0.2
    priv = torch.randn(rows, PRIV, generator=g)
    noise = torch.randn(rows, 6, generator=g)
    p64 = {k: v.double() for k, v in init.items()}

    def norm64(x, mean, var):     # running_mean_std.py:91-92
        return torch.clamp((x.double() - mean) / torch.sqrt(var + 1e-5), -5.0, 5.0)

    def ref(normalize):
        o = norm64(obs, mean_o, var_o) if normalize else obs.double()
        q = norm64(priv, mean_p, var_p) if normalize else priv.double()
        with torch.no_grad():
            return sr.actor_critic(p64, o, q, len(priv_units), len(units))
    return eng, obs, priv, noise, ref, obs_dim, priv_units


@pytest.mark.parametrize("rows", [80, 300])      # two 32-row blocks and a ragged one; more rows than mb = 256
@pytest.mark.parametrize("case", list(INFER_CASES))
def test_shared_infer_matches_float64(case, rows):
    eng, obs, priv, _, ref, obs_dim, priv_units = _infer_setup(case, rows)
    for normalize in (True, False):
        mu, val, lat = eng.infer(obs, priv, want_latent=True, normalize=normalize)
        torch.cuda.synchronize()
        m, _, v, e = ref(normalize)
        assert lat.shape == (rows, priv_units[-1])
        np.testing.assert_allclose(mu.cpu().numpy(), m.numpy(), atol=2e-6, rtol=1e-4)
        np.testing.assert_allclose(val.cpu().numpy(), v.numpy(), atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(lat.cpu().numpy(), e.numpy(), atol=2e-6, rtol=1e-4)


@pytest.mark.parametrize("rows", [80, 300])
@pytest.mark.parametrize("case", list(INFER_CASES))
def test_shared_rollout_policy_step_matches_float64(case, rows):
    """rollout_policy_step on given noise against a float64 restatement of model_act + the storage writes of play_steps, at
    the bounds of tests/test_gpu_teacher_shapes.py's policy-step test."""
    from oracle import teacher as ot
    eng, obs, priv, noise, ref, obs_dim, _ = _infer_setup(case, rows)
    f = dict(dtype=torch.float32, device="cuda:0")
    n = rows
    o = dict(obses=torch.zeros(n, obs_dim, **f), priv=torch.zeros(n, PRIV, **f), actions=torch.zeros(n, 6, **f),
             nlp=torch.zeros(n, **f), values=torch.zeros(n, 1, **f), mus=torch.zeros(n, 6, **f),
             sigmas=torch.zeros(n, 6, **f), clamped=torch.zeros(n, 6, **f), vout=torch.zeros(n, 1, **f))
    rms_v = torch.tensor([0.5, 4.0, 100.0], dtype=torch.float64, device="cuda:0")
    torch.ops.mi355ppo.rollout_policy_step(eng.state_list(), *eng._cfg_args(), obs.cuda(), priv.cuda(), True, noise.cuda(),
                                           rms_v, o["obses"], o["priv"], o["actions"], o["nlp"], o["values"], o["mus"],
                                           o["sigmas"], o["clamped"], o["vout"])
    torch.cuda.synchronize()
    mu, logstd, value, _ = ref(True)
    sigma = torch.exp(logstd)
    action = mu + sigma * noise.double()
    nlp = ot.gaussian_neglogp(action, mu, sigma, logstd)
    value = np.sqrt(4.0 + 1e-5) * torch.clamp(value, -5.0, 5.0) + 0.5
    assert torch.equal(o["obses"].cpu(), obs) and torch.equal(o["priv"].cpu(), priv)
    for k, want, atol in (("mus", mu, 2e-5), ("sigmas", sigma, 1e-6), ("actions", action, 2e-5),
                          ("clamped", action.clamp(-1.0, 1.0), 2e-5), ("values", value, 2e-5), ("vout", value, 2e-5),
                          ("nlp", nlp, 5e-5)):
        np.testing.assert_allclose(o[k].cpu().numpy(), want.numpy(), atol=atol, rtol=1e-5, err_msg=k)


# ---- 7. bit-level properties ----------------------------------------------------------------------------------------
BIT_CASES = {"default_mb256": ((64, 8, 2), DEFAULT_UNITS, DEFAULT_PRIV_UNITS), "small_mb200": ((100, 6, 3), SMALL_UNITS, SMALL_PRIV_UNITS)}


def _snapshot(eng):
    torch.cuda.synchronize()
    return [t.clone() for t in (eng.params, eng.stats, eng.adam_m, eng.adam_v, eng.mus_w, eng.sigmas_w, eng.rms_obs,
                                eng.rms_priv, eng.grads)]


@pytest.mark.parametrize("case", list(BIT_CASES))
def test_shared_update_drivers_give_the_same_bits(case):
    """The same update twice; the whole update against the step-wise loop; the two-phase schedule against the unsplit
    step (every gradient range assembled exactly once); a one-rank RCCL update against the single-GPU one."""
    from isaacgyminsertion_amd.utils.dist import NativeComm
    (N, T, Ep), units, priv_units = BIT_CASES[case]
    init, ro, perm = sr.problem(N, T, units, priv_units, seed=21)
    ro = {k: v.cuda() for k, v in ro.items()}
    torch.cuda.set_device(0)

    def run(how, comm=None):
        eng = _engine(N, T, Ep, units, priv_units, init, perm)
        for v in eng.param_views(eng.grads).values():
            v.fill_(float("nan"))               # a range no phase assembles would keep its NaN (the alignment gaps stay zero)
        eng.prepare(ro)
        if how == "whole":
            eng.update()
        elif how in ("overlap", "serial"):
            eng.update_dp_native(comm, overlap=(how == "overlap"))
        else:
            slot = 0
            for _ in range(Ep):
                for i in range(eng.n_mb):
                    if how == "phased":
                        eng.fwd_bwd_phase(i, slot, 0)
                        eng.fwd_bwd_phase(i, slot, 1)
                    else:
                        eng.fwd_bwd(i, slot)
                    eng.apply(slot)
                    slot += 1
        return _snapshot(eng)

    ref = run("whole")
    assert all(torch.isfinite(t).all() for t in ref)
    comm = NativeComm(rank=0, world=1)
    try:
        for how in ("whole", "stepwise", "phased", "overlap", "serial"):
            got = run(how, comm)
            for j, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(a, b), (how, j)
    finally:
        comm.close()


def test_shared_update_under_the_schedule_and_the_early_stop():
    """lr_schedule="adaptive" and kl_early_stop=True, one case each: the whole update's stop step, estimator sequence,
    rate record and bits equal the step-wise loop's.  (lr = 5e-3: the first step moves mu by far more than either
    threshold allows, so the stop is at a step >= 1 -- step 0's estimator is 0 up to rounding -- and the rate moves.)"""
    N, T, Ep = 64, 8, 4
    init, ro, perm = sr.problem(N, T, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, seed=5)
    ro = {k: v.cuda() for k, v in ro.items()}
    for kw in (dict(kl_early_stop=True, kl_threshold=1e-3), dict(lr_schedule="adaptive", kl_threshold=1e-3)):
        out = []
        for how in ("whole", "stepwise"):
            eng = _engine(N, T, Ep, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, init, perm, lr=5e-3, **kw)
            eng.prepare(ro)
            if how == "whole":
                eng.update()
            else:
                slot = 0
                for _ in range(Ep):
                    for i in range(eng.n_mb):
                        eng.fwd_bwd(i, slot)
                        eng.apply(slot)
                        slot += 1
            snap = _snapshot(eng)[:8]
            if eng.kl_early_stop:
                rec = (eng.stop_step, eng.approx_kl(), eng.adam_t)
                assert rec[0] is not None and 1 <= rec[0] < Ep * eng.n_mb and rec[2] == rec[0]
            else:
                rec = (eng.lr_history(), eng.lr)
                assert rec[1] < 5e-3
            out.append((snap, rec))
        (sa, ra), (sb, rb) = out
        for j, (a, b) in enumerate(zip(sa, sb)):
            n = ra[0] if kw.get("kl_early_stop") and j == 1 else None      # statistics rows behind the stop are never read
            assert torch.equal(a[:n], b[:n]), (kw, j)
        assert ra[0] == rb[0] if kw.get("kl_early_stop") else torch.equal(ra[0], rb[0])
        assert torch.equal(ra[1], rb[1]) if kw.get("kl_early_stop") else ra[1] == rb[1]


def test_switch_off_is_the_engine_without_the_argument():
    """shared_parameters=False: step-0 gradient and first update bit-equal to an engine built without the argument."""
    N, T, Ep = 64, 8, 2
    from oracle import synth
    init, ro, perm = synth.teacher_problem(N, T, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, seed=3, done_p=0.05)
    ro = {k: v.cuda() for k, v in ro.items()}
    out = []
    for shared in (None, False):
        eng = _engine(N, T, Ep, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, init, perm, shared=shared)
        assert not eng.shared_parameters and len(eng.shapes) == 23
        eng.prepare(ro)
        eng.fwd_bwd(0, 0)
        torch.cuda.synchronize()
        g0 = eng.grads.clone()
        eng.prepare(ro)
        eng.update()
        out.append([g0] + _snapshot(eng))
    for j, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), j


# ---- 8. through the trainers -------------------------------------------------------------------------------------------
def _ppo(num_envs, horizon, mini_epochs, env=None, out=None, units=SMALL_UNITS, priv_units=SMALL_PRIV_UNITS):
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=num_envs, horizon_length=horizon, rl_device="cuda:0", mini_epochs=mini_epochs,
                         num_points=8, shared_parameters=True)
    cfg.train.network.mlp.units = list(units)
    cfg.train.network.priv_mlp.units = list(priv_units)
    return PPO(env, out, cfg), cfg


def test_ppo_trains_and_round_trips_a_shared_teacher(tmp_path):
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    N, T = 64, 8
    env = SyntheticInsertionEnv(N, device="cuda:0")
    agent, _ = _ppo(N, T, 4, env=env, out=str(tmp_path), units=DEFAULT_UNITS, priv_units=DEFAULT_PRIV_UNITS)
    assert agent.engine.shared_parameters and not hasattr(agent.model, "critic_mlp")
    assert sum(p.numel() for p in agent.model.parameters()) == 227989
    agent.obs = env.reset()
    before = agent.engine.params.clone()
    a_losses, c_losses, b_losses, entropies, kls, grad_norms, _ = agent.train_epoch()      # play_steps + update
    torch.cuda.synchronize()
    assert len(a_losses) == 16
    for lst in (a_losses, c_losses, b_losses, entropies, kls, grad_norms):
        assert all(torch.isfinite(x) for x in lst)
    assert torch.isfinite(agent.engine.params).all() and not torch.equal(before, agent.engine.params)
    agent.save(str(tmp_path / "mine"))
    ck = torch.load(str(tmp_path / "mine.pth"), map_location="cpu")
    assert len(ck["model"]) == 17 and not any(k.startswith("critic_mlp") for k in ck["model"])
    other, _ = _ppo(N, T, 4, units=DEFAULT_UNITS, priv_units=DEFAULT_PRIV_UNITS)
    other.restore_train(str(tmp_path / "mine.pth"))
    assert torch.equal(other.engine.params, agent.engine.params)
    assert torch.equal(other.engine.rms_obs, agent.engine.rms_obs) and torch.equal(other.engine.rms_priv, agent.engine.rms_priv)


def test_reference_written_shared_checkpoint_loads_and_tests(tmp_path):
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    ck, units, priv_units = sr.load_ckpt()
    path = str(tmp_path / "ref.pth")
    torch.save(ck, path)
    env = SyntheticInsertionEnv(32, device="cuda:0")
    agent, _ = _ppo(32, 8, 4, env=env, units=units, priv_units=priv_units)
    agent.restore_test(path)
    sd = agent.model.state_dict()
    assert list(sd.keys()) == list(ck["model"].keys())
    for k, v in ck["model"].items():
        assert torch.equal(sd[k].cpu(), v), k
    np.testing.assert_array_equal(agent.running_mean_std.state_dict()["running_mean"].cpu().numpy(),
                                  ck["running_mean_std"]["running_mean"].numpy())
    # the engine sees the restored weights: inference equals the float64 restatement
    g = torch.Generator().manual_seed(0)
    obs, priv = torch.randn(20, 15, generator=g), torch.randn(20, 64, generator=g)
    mu, _ = agent.model.act_inference({"obs": obs.cuda(), "priv_info": priv.cuda()})
    p = {k: v.double() for k, v in ck["model"].items()}
    with torch.no_grad():
        mu_ref, _, _, _ = sr.actor_critic(p, obs.double(), priv.double(), len(priv_units), len(units))
    np.testing.assert_allclose(mu.cpu().numpy(), mu_ref.numpy(), atol=1e-5)
    agent.test(total_steps=8)
    torch.cuda.synchronize()


def test_extrinsic_adapt_runs_on_a_restored_shared_teacher(tmp_path):
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    ck, units, priv_units = sr.load_ckpt()
    path = str(tmp_path / "ref.pth")
    torch.save(ck, path)
    n, T = 8, 4
    cfg = default_config(num_envs=n, horizon_length=T, rl_device="cuda:0", mini_epochs=2, obs_info=True, num_points=8,
                         shared_parameters=True)
    cfg.train.network.mlp.units = list(units)
    cfg.train.network.priv_mlp.units = list(priv_units)
    env = SyntheticInsertionEnv(n, device="cuda:0")
    agent = ExtrinsicAdapt(env, str(tmp_path), cfg)
    agent.restore_train(path)
    assert agent.agent.shared_parameters and not hasattr(agent.agent, "critic_mlp")
    for k, v in ck["model"].items():
        assert torch.equal(agent.agent.state_dict()[k].cpu(), v), k
    teacher_before = agent.agent.flat_params.clone()
    agent.obs = env.reset()
    a1, _ = agent.train_epoch()                                        # play_steps + the student update
    assert len(a1) > 0 and all(torch.isfinite(x) for x in a1)
    assert torch.equal(agent.agent.flat_params, teacher_before)      # inference only: the teacher stays frozen


# ---- the two registrations ---------------------------------------------------------------------------------------------
def test_cpp_and_python_registrations_agree_on_a_shared_teacher(tmp_path):
    lib = os.path.join(ROOT, "isaacgyminsertion_amd", "libigi_torch_ops.so")
    if not os.path.exists(lib):
        pytest.skip("libigi_torch_ops.so not built on this host (python -c 'import __graft_entry__ as g; g.build()')")
    child = os.path.join(ROOT, "tests", "cpp_ops_shared_child.py")
    paths = {}
    for which in ("cpp", "py"):
        paths[which] = str(tmp_path / f"{which}.npz")
        r = subprocess.run([sys.executable, child, "run", which, paths[which]], cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    A, B = np.load(paths["cpp"]), np.load(paths["py"])
    assert set(A.files) == set(B.files)
    for k in A.files:
        assert A[k].shape == B[k].shape and np.array_equal(A[k], B[k]), k
    assert list(A["refused"]) == [1, 1, 1] and int(A["stop"][0]) == -1
    assert np.isfinite(A["params_after2"]).all() and np.abs(A["params_after2"] - A["params_after"]).max() > 0
