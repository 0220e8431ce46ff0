"""Rollout bookkeeping (igi_teacher_infer + igi_rollout_act_store + igi_rollout_env_store behind PPO.play_steps
and ExtrinsicAdapt.play_steps) against golden vectors captured from the REFERENCE's own play_steps
(frozen_ppo.py:648-725, ext_adapt.py:658-767) driven by a scripted environment with pre-drawn Gaussian noise
(tests/golden/make_golden_rollout.py).

Tolerances (fp32 network outputs vs ATen on CPU): policy outputs / stored values 2e-5 abs, neglogp 5e-5 abs (six
squared terms scaled by 1/(2 sigma^2)), everything that is pure bookkeeping (observations, dones, accumulators,
meter sizes, agent_steps) exact; shaped rewards and meters inherit the value tolerance."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout.npz"))
DEV = "cuda:0"


class ScriptedEnv:
    """Replays the fixture's pre-drawn step results on the device; records the actions it is given."""

    def __init__(self, script, extra=(), **queues):
        self.s = {k: torch.from_numpy(v).to(DEV) for k, v in script.items()}
        self.extra = tuple(extra)
        self.t = 0
        self.actions = []
        self.num_envs = self.s["obs"].shape[1]
        for k, v in queues.items():
            setattr(self, k, v)

    def obs(self):
        d = {"obs": self.s["obs"][self.t], "priv_info": self.s["priv_info"][self.t]}
        for k in self.extra:
            d[k] = self.s[k][self.t]
        return d

    def reset(self, **k):
        self.t = 0
        return self.obs()

    def step(self, actions):
        self.actions.append(actions.clone())
        t = self.t
        self.t += 1
        infos = {"time_outs": self.s["time_outs"][t], "successes": self.s["successes"][t], "scalar_metric": 0.5 + t}
        return self.obs(), self.s["rewards"][t], self.s["dones"][t], infos


class ReplayNoise:
    """torch.randn_like -> the fixture's noise[call index] (the product draws its exploration noise there)."""

    def __init__(self, monkeypatch, noise):
        self.noise = torch.from_numpy(noise).to(DEV)
        self.i = 0
        monkeypatch.setattr(torch, "randn_like", self)

    def __call__(self, t, **k):
        e = self.noise[self.i]
        self.i += 1
        assert e.shape == t.shape
        return e


def _script(prefix):
    return {k[len(prefix):]: G[k] for k in G.files if k.startswith(prefix)}


def _load_rms(module, packed):
    d = (packed.size - 1) // 2
    module.load_state_dict({"running_mean": torch.from_numpy(packed[:d].copy()),
                            "running_var": torch.from_numpy(packed[d:2 * d].copy()),
                            "count": torch.tensor(packed[2 * d])})


def _rms_state(m):
    return np.concatenate([m.running_mean.cpu().numpy().reshape(-1), m.running_var.cpu().numpy().reshape(-1),
                           np.array([m.count.item()])])


def test_ppo_play_steps_matches_reference(monkeypatch):
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.utils.config import default_config
    N, T, R = [int(x) for x in G["ppo/meta"]]
    cfg = default_config(num_envs=N, horizon_length=T, rl_device=DEV, mini_epochs=2, num_points=8)
    cfg.train.network.mlp.units = [int(x) for x in G["ppo/units"]]
    cfg.train.network.priv_mlp.units = [int(x) for x in G["ppo/priv_units"]]
    env = ScriptedEnv(_script("ppo/r0/script/"))
    agent = PPO(env, None, cfg)
    agent.model.load_state_dict({k[len("ppo/init/"):]: torch.from_numpy(G[k]) for k in G.files
                                 if k.startswith("ppo/init/")})
    for nm in ("running_mean_std", "priv_mean_std", "value_mean_std"):
        _load_rms(getattr(agent, nm), G[f"ppo/rms_in/{nm}"])
    agent.set_eval()
    agent.agent_steps = agent.batch_size
    for r in range(R):
        sc = _script(f"ppo/r{r}/script/")
        env.__init__(sc)
        agent.obs = env.reset()
        ReplayNoise(monkeypatch, sc["noise"])
        agent.play_steps()
        torch.cuda.synchronize()
        sd = agent.storage.storage_dict
        ref = lambda k: G[f"ppo/r{r}/{k}"]                      # noqa: E731
        for k in ("obses", "priv_info", "dones"):
            assert np.array_equal(sd[k].cpu().numpy(), ref(f"storage/{k}")), k
        for k, atol in (("mus", 2e-5), ("sigmas", 1e-6), ("actions", 2e-5), ("values", 2e-5), ("neglogpacs", 5e-5),
                        ("rewards", 2e-5), ("returns", 1e-4)):
            np.testing.assert_allclose(sd[k].cpu().numpy(), ref(f"storage/{k}"), atol=atol, rtol=1e-5, err_msg=k)
        got_act = torch.stack(env.actions).cpu().numpy()
        np.testing.assert_allclose(got_act, ref("env_actions"), atol=2e-5)       # clamp(actions, +-1) reaches the env
        assert np.abs(got_act).max() <= 1.0 and (np.abs(ref("storage/actions")) > 1).any()
        np.testing.assert_allclose(agent.current_rewards.cpu().numpy().reshape(-1), ref("current_rewards").reshape(-1), atol=1e-6)
        assert np.array_equal(agent.current_lengths.cpu().numpy().reshape(-1), ref("current_lengths").reshape(-1))
        assert np.array_equal(agent.current_success.cpu().numpy().reshape(-1), ref("current_success").reshape(-1))
        for nm in ("episode_rewards", "episode_lengths", "episode_success"):
            m = getattr(agent, nm)
            np.testing.assert_allclose([m.get_mean(), len(m)], ref(f"meter/{nm}"), rtol=1e-5, atol=1e-6, err_msg=nm)
        # the post-rollout tail: GAE, advantage normalisation, the two value_mean_std updates
        np.testing.assert_allclose(agent.storage.data_dict["advantages"].cpu().numpy(), ref("advantages"), atol=2e-4)
        np.testing.assert_allclose(agent.storage.data_dict["values"].cpu().numpy(), ref("values_norm"), atol=5e-5)
        np.testing.assert_allclose(agent.storage.data_dict["returns"].cpu().numpy(), ref("returns_norm"), atol=1e-4)
        np.testing.assert_allclose(_rms_state(agent.value_mean_std), ref("value_mean_std"), rtol=1e-5)
        assert agent.agent_steps == int(ref("agent_steps"))
        assert float(agent.extra_info["scalar_metric"]) == float(ref("extra_info"))
    for nm in ("running_mean_std", "priv_mean_std"):            # eval mode during the rollout: untouched
        assert np.array_equal(_rms_state(getattr(agent, nm)), G[f"ppo/rms_in/{nm}"])


@pytest.mark.parametrize("tag", ["s2_lin", "s2_tac_pcl"])
def test_student_play_steps_matches_reference(tag, monkeypatch):
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.utils.config import default_config
    N, T, tactile, pcl, steps0 = [int(x) for x in G[f"{tag}/meta"]]
    cfg = default_config(num_envs=N, horizon_length=T, rl_device=DEV, mini_epochs=2, obs_info=True,
                         tactile_info=bool(tactile), pcl_info=bool(pcl), num_points=8)
    cfg.offline_train.only_bc = True
    sc = _script(f"{tag}/script/")
    extra = ["student_obs"] + (["tactile"] if tactile else []) + (["pcl"] if pcl else [])
    env = ScriptedEnv(sc, extra,
                      tactile_queue=torch.zeros(N, 1, 3, 2048, device=DEV) if tactile else None,
                      pcl_queue=torch.zeros(N, 1, 2400, device=DEV) if pcl else None, img_queue=None, seg_queue=None)
    agent = ExtrinsicAdapt(env, None, cfg)
    agent.student.model.load_state_dict({k[len(tag) + 9:]: torch.from_numpy(G[k]) for k in G.files
                                         if k.startswith(f"{tag}/student/")})
    agent.agent.load_state_dict({k[len(tag) + 9:]: torch.from_numpy(G[k]) for k in G.files
                                 if k.startswith(f"{tag}/teacher/")})
    rms_names = ("running_mean_std", "priv_mean_std", "stud_obs_mean_std") + (("pcl_mean_std",) if pcl else ())
    for nm in rms_names:
        _load_rms(getattr(agent, nm), G[f"{tag}/rms_in/{nm}"])
    agent.set_student_eval()
    agent.agent_steps = steps0
    agent.obs = env.reset()
    ReplayNoise(monkeypatch, sc["noise"])
    agent.play_steps()
    torch.cuda.synchronize()
    sd = agent.storage.storage_dict
    tol = {"n_obs": 1e-6, "n_priv_info": 1e-6, "n_student_obs": 2e-6, "n_pcl": 2e-5, "n_tactile": 0.0,
           "latent_gt": 2e-5, "teacher_actions": 2e-5, "student_actions": 5e-5, "rewards": 2e-5}
    for k in [f[len(tag) + 9:] for f in G.files if f.startswith(f"{tag}/storage/")]:
        np.testing.assert_allclose(sd[k].cpu().numpy(), G[f"{tag}/storage/{k}"], atol=tol[k], rtol=1e-5, err_msg=k)
    got_act = torch.stack(env.actions).cpu().numpy()
    np.testing.assert_allclose(got_act, G[f"{tag}/env_actions"], atol=5e-5)
    who = "student_actions" if tactile else "teacher_actions"     # DAgger beta = 0 past 3e6 steps (ext_adapt.py:718-728)
    np.testing.assert_allclose(got_act, np.clip(G[f"{tag}/storage/{who}"], -1, 1), atol=5e-5)
    np.testing.assert_allclose(agent.step_reward.cpu().numpy().reshape(-1), G[f"{tag}/step_reward"].reshape(-1), atol=1e-6)
    assert np.array_equal(agent.step_length.cpu().numpy().reshape(-1), G[f"{tag}/step_length"].reshape(-1))
    assert np.array_equal(agent.step_success.cpu().numpy().reshape(-1), G[f"{tag}/step_success"].reshape(-1))
    for nm in ("mean_eps_reward", "mean_eps_length", "mean_eps_success"):
        m = getattr(agent, nm)
        np.testing.assert_allclose([m.get_mean(), len(m)], G[f"{tag}/meter/{nm}"], rtol=1e-5, atol=1e-6, err_msg=nm)
    for nm in rms_names:      # stud_obs / pcl normalisers are in TRAIN mode during the rollout
        np.testing.assert_allclose(_rms_state(getattr(agent, nm)), G[f"{tag}/rms_out/{nm}"], rtol=1e-5, atol=1e-8,
                                   err_msg=nm)
    assert agent.agent_steps == int(G[f"{tag}/agent_steps"])


def test_fused_policy_step_equals_infer_plus_act_store():
    """torch.ops.mi355ppo.rollout_policy_step (one native call per environment step: normalise + forward + sample +
    arena writes) against the two ops it fuses -- actor_critic_infer and rollout_act_store, the pair the reference
    goldens above pin -- on the same inputs, noise and normaliser states, at the rollout's 4096 rows and at 10,007 rows
    (ragged last 32-row block).  Round 6: the step is the persistent policy kernel (csrc/policy_fwd.h: stage + ONE launch)
    while actor_critic_infer stays layer by layer, so the comparison is at fp32 rounding instead of bit for bit -- the
    trunk layers keep the GEMM kernels' k order (bit-identical), the 8-wide latent layer and the heads sum their 128
    terms in another order: raw copies exact, means / values / actions 2e-6 (measured below 1e-6), neglogp 2e-5 relative
    (it divides by sigma^2).  The profiler confirms which kernel ran."""
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from oracle import synth
    units, priv_units = [512, 256, 128], [256, 128, 8]
    from isaacgyminsertion_amd import _lib
    for N, T in ((4096, 8), (10007, 4)):
        init, ro, perm = synth.teacher_problem(64, 4, units, priv_units, seed=5)
        eng = TeacherEngine(N, T, 4, units=units, priv_units=priv_units, device="cuda:0")
        eng.load_params(init)
        g = torch.Generator(device="cuda:0").manual_seed(N)
        obs = torch.randn(N, 15, device="cuda:0", generator=g) * 2 + 0.3
        priv = torch.randn(N, 64, device="cuda:0", generator=g)
        noise = torch.randn(N, 6, device="cuda:0", generator=g)
        eng.rms_obs[:15] = 0.3; eng.rms_obs[15:30] = 3.0
        eng.rms_priv[:64] = torch.linspace(-1, 1, 64, dtype=torch.float64, device="cuda:0")
        rms_v = torch.tensor([0.5, 4.0, 100.0], dtype=torch.float64, device="cuda:0")
        f = dict(dtype=torch.float32, device="cuda:0")

        def outs():
            return dict(obses=torch.zeros(N, 15, **f), priv=torch.zeros(N, 64, **f), actions=torch.zeros(N, 6, **f),
                        nlp=torch.zeros(N, **f), values=torch.zeros(N, 1, **f), mus=torch.zeros(N, 6, **f),
                        sigmas=torch.zeros(N, 6, **f), clamped=torch.zeros(N, 6, **f), vout=torch.zeros(N, 1, **f))

        a, b = outs(), outs()
        mu, value_n = eng.infer(obs, priv, normalize=True)
        torch.ops.mi355ppo.rollout_act_store(obs, priv, mu, value_n, eng.param_views()["sigma"], noise, rms_v, 1e-5,
                                             a["obses"], a["priv"], a["actions"], a["nlp"], a["values"], a["mus"],
                                             a["sigmas"], a["clamped"], a["vout"])
        _lib.prof_enable(True)
        try:
            torch.ops.mi355ppo.rollout_policy_step(eng.state_list(), *eng._cfg_args(), obs, priv, True, noise, rms_v,
                                                   b["obses"], b["priv"], b["actions"], b["nlp"], b["values"], b["mus"],
                                                   b["sigmas"], b["clamped"], b["vout"])
            torch.cuda.synchronize()
            classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
        finally:
            _lib.prof_enable(False)
        assert classes.get("k_policy_fwd", 0) == 1, classes
        for k in ("obses", "priv", "sigmas"):
            assert torch.equal(a[k], b[k]), (N, k)
        for k in ("mus", "actions", "clamped", "values", "vout"):
            np.testing.assert_allclose(b[k].cpu().numpy(), a[k].cpu().numpy(), atol=2e-6, rtol=2e-6, err_msg=f"{N} {k}")
        np.testing.assert_allclose(b["nlp"].cpu().numpy(), a["nlp"].cpu().numpy(), rtol=2e-5, atol=2e-5, err_msg=f"{N} nlp")
        assert torch.isfinite(b["nlp"]).all() and float(b["actions"].abs().max()) > 0


@pytest.mark.parametrize("N,obs_dim,act_dim", [(100, 11, 3), (33, 15, 7), (1, 24, 6), (4100, 15, 6)])
def test_persistent_policy_kernel_on_other_widths_and_ragged_row_counts(N, obs_dim, act_dim):
    """k_policy_fwd (csrc/policy_fwd.h) takes any observation width up to 24 and up to 7 actions with the reference's layer
    sizes, and any row count (32-row blocks, the last one ragged): against actor_critic_infer + rollout_act_store (the
    layer-by-layer launches) at fp32 rounding, and the profiler confirms that the persistent kernel ran."""
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from oracle import synth
    units, priv_units = [512, 256, 128], [256, 128, 8]
    init, ro, perm = synth.teacher_problem(64, 4, units, priv_units, obs_dim=obs_dim, act_dim=act_dim, seed=9)
    eng = TeacherEngine(max(N, 64), 4, 2, units=units, priv_units=priv_units, obs_dim=obs_dim, act_dim=act_dim, device="cuda:0")
    eng.load_params(init)
    g = torch.Generator(device="cuda:0").manual_seed(N)
    f = dict(dtype=torch.float32, device="cuda:0")
    obs = torch.randn(N, obs_dim, device="cuda:0", generator=g) * 1.5
    priv = torch.randn(N, 64, device="cuda:0", generator=g)
    noise = torch.randn(N, act_dim, device="cuda:0", generator=g)
    rms_v = torch.tensor([0.2, 2.0, 50.0], dtype=torch.float64, device="cuda:0")

    def outs():
        return dict(obses=torch.zeros(N, obs_dim, **f), priv=torch.zeros(N, 64, **f), actions=torch.zeros(N, act_dim, **f),
                    nlp=torch.zeros(N, **f), values=torch.zeros(N, 1, **f), mus=torch.zeros(N, act_dim, **f),
                    sigmas=torch.zeros(N, act_dim, **f), clamped=torch.zeros(N, act_dim, **f), vout=torch.zeros(N, 1, **f))

    a, b = outs(), outs()
    mu, value_n = eng.infer(obs, priv, normalize=True)
    torch.ops.mi355ppo.rollout_act_store(obs, priv, mu, value_n, eng.param_views()["sigma"], noise, rms_v, 1e-5,
                                         a["obses"], a["priv"], a["actions"], a["nlp"], a["values"], a["mus"],
                                         a["sigmas"], a["clamped"], a["vout"])
    _lib.prof_enable(True)
    try:
        torch.ops.mi355ppo.rollout_policy_step(eng.state_list(), *eng._cfg_args(), obs, priv, True, noise, rms_v,
                                               b["obses"], b["priv"], b["actions"], b["nlp"], b["values"], b["mus"],
                                               b["sigmas"], b["clamped"], b["vout"])
        torch.cuda.synchronize()
        classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    assert classes.get("k_policy_fwd", 0) == 1, classes
    for k in ("obses", "priv", "sigmas"):
        assert torch.equal(a[k], b[k]), k
    for k in ("mus", "actions", "clamped", "values", "vout"):
        np.testing.assert_allclose(b[k].cpu().numpy(), a[k].cpu().numpy(), atol=2e-6, rtol=2e-6, err_msg=k)
    np.testing.assert_allclose(b["nlp"].cpu().numpy(), a["nlp"].cpu().numpy(), rtol=2e-5, atol=2e-5)
