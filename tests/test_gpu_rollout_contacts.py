"""The contact teacher's rollout policy step in the persistent policy kernel (csrc/policy_fwd.h, contact mode): with the
reference's layer sizes and xcat = [obs | latent 8 | embedding] (or [obs | embedding] with only_contact) no wider than 32
columns, rollout_policy_step_contacts is k_policy_stage + ONE k_policy_fwd launch per chunk of mb rows -- contact encoder,
env_mlp, both trunks, the heads, the Normal sample and every arena write, the raw contacts among them.

Checked against float64 (oracle/teacher.py actor_critic + the sample on the given noise), against the layer-by-layer
launches (infer_contacts + rollout_act_store) on the same inputs, against the reference's own model_act at the default
network (tests/golden/rollout_contacts_default.npz), and through the trainer's play_steps.  The profiler classes say which
kernels ran, so a case cannot silently fall back to the layer-by-layer path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRIV = 64
UNITS, PRIV_UNITS = [512, 256, 128], [256, 128, 8]
HERE = os.path.dirname(os.path.abspath(__file__))


def _classes(fn):
    """{profiler class: launches} of the native calls fn makes"""
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        classes = {}
        for c in _lib.prof_read():
            name = c["name"].split(":")[0]
            classes[name] = classes.get(name, 0) + c["launches"]
    finally:
        _lib.prof_enable(False)
    return {k: v for k, v in classes.items() if v}


def _outs(n, obs_dim, act, P):
    f = dict(dtype=torch.float32, device="cuda:0")
    return dict(obses=torch.zeros(n, obs_dim, **f), priv=torch.zeros(n, PRIV, **f), contacts=torch.zeros(n, max(P, 1), **f),
                actions=torch.zeros(n, act, **f), nlp=torch.zeros(n, **f), values=torch.zeros(n, 1, **f),
                mus=torch.zeros(n, act, **f), sigmas=torch.zeros(n, act, **f), clamped=torch.zeros(n, act, **f),
                vout=torch.zeros(n, 1, **f))


def _step(eng, d, o, rms_v):
    """the rollout policy step of `eng` on the device inputs d into the arena slot / outputs o"""
    if eng.contact_points:
        torch.ops.mi355ppo.rollout_policy_step_contacts(eng.state_list(), *eng._cfg_args(), d["obs"], d["priv"], d["contacts"],
                                                        True, d["noise"], rms_v, o["obses"], o["priv"], o["contacts"],
                                                        o["actions"], o["nlp"], o["values"], o["mus"], o["sigmas"],
                                                        o["clamped"], o["vout"])
    else:
        torch.ops.mi355ppo.rollout_policy_step(eng.state_list(), *eng._cfg_args(), d["obs"], d["priv"], True, d["noise"],
                                               rms_v, o["obses"], o["priv"], o["actions"], o["nlp"], o["values"], o["mus"],
                                               o["sigmas"], o["clamped"], o["vout"])


def _setup(rows, obs_dim, act, P, E, oc, engine=None, real_contacts=False):
    """An engine with the default network and random parameters (biases and sigma away from zero), running statistics away
    from (0, 1), inputs as _infer_setup of tests/test_gpu_teacher_shapes.py draws them, and the float64 reference."""
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from oracle import teacher as ot
    g = torch.Generator().manual_seed(1000 * rows + 10 * P + E + int(oc))
    init = {}
    for k, shp in ot.teacher_param_shapes(obs_dim, PRIV, act, UNITS, PRIV_UNITS, P, E, oc).items():
        init[k] = torch.randn(*shp, generator=g) / np.sqrt(shp[1]) if len(shp) == 2 else 0.05 * torch.randn(*shp, generator=g)
    init["sigma"] = 0.3 * torch.randn(act, generator=g)
    N, T, Ep = engine or (max(rows, 64), 4, 2)
    eng = TeacherEngine(N, T, Ep, units=UNITS, priv_units=PRIV_UNITS, obs_dim=obs_dim, act_dim=act, contact_points=P,
                        contact_emb=E, only_contact=oc)
    eng.load_params(init)
    mean_o, var_o = 0.3 * torch.randn(obs_dim, generator=g).double(), (0.5 + torch.rand(obs_dim, generator=g)).double()
    mean_p, var_p = 0.3 * torch.randn(PRIV, generator=g).double(), (0.5 + torch.rand(PRIV, generator=g)).double()
    eng.rms_obs[:obs_dim], eng.rms_obs[obs_dim:2 * obs_dim] = mean_o.cuda(), var_o.cuda()
    eng.rms_priv[:PRIV], eng.rms_priv[PRIV:2 * PRIV] = mean_p.cuda(), var_p.cuda()
    x = dict(obs=1.5 * torch.randn(rows, obs_dim, generator=g) + 0.2, priv=torch.randn(rows, PRIV, generator=g))
    if P:
        x["contacts"] = torch.randn(rows, P, generator=g) if real_contacts else (torch.rand(rows, P, generator=g) < 0.2).float()
    x["noise"] = torch.randn(rows, act, generator=g)
    p64 = {k: v.double() for k, v in init.items()}

    def norm64(v, mean, var):     # running_mean_std.py:91-92
        return torch.clamp((v.double() - mean) / torch.sqrt(var + 1e-5), -5.0, 5.0)

    def ref():
        """float64: model_act + the storage writes of play_steps (frozen_ppo.py:343-366, 655-665) on the given noise"""
        with torch.no_grad():
            mu, logstd, value, _ = ot.actor_critic(p64, norm64(x["obs"], mean_o, var_o), norm64(x["priv"], mean_p, var_p),
                                                   len(PRIV_UNITS), len(UNITS), x["contacts"].double() if P else None, oc)
        sigma = torch.exp(logstd)
        action = mu + sigma * x["noise"].double()
        value = np.sqrt(4.0 + 1e-5) * torch.clamp(value, -5.0, 5.0) + 0.5        # value_mean_std(values, unnorm=True)
        return dict(mus=mu, sigmas=sigma.expand_as(mu), actions=action, clamped=action.clamp(-1.0, 1.0), values=value,
                    vout=value, nlp=ot.gaussian_neglogp(action, mu, sigma, logstd))
    return eng, x, {k: v.cuda() for k, v in x.items()}, ref


RMS_V = [0.5, 4.0, 100.0]
# the bounds of test_rollout_policy_step_off_the_default_widths_matches_float64 (tests/test_gpu_teacher_shapes.py)
F64_ATOL = dict(mus=2e-5, sigmas=1e-6, actions=2e-5, clamped=2e-5, values=2e-5, vout=2e-5, nlp=5e-5)


def _assert_f64(o, want, tag=""):
    for k, atol in F64_ATOL.items():
        got = o[k].cpu().numpy()
        print(f"{tag}{k}: max |fp32 - fp64| = {np.abs(got - want[k].numpy()).max():.3e}")
        np.testing.assert_allclose(got, want[k].numpy(), atol=atol, rtol=1e-5, err_msg=k)


CASES = [
    # rows, obs, act, P, E, only_contact, engine (N, T, mini_epochs) or None, real-valued contacts
    (80, 15, 6, 400, 8, False, None, False),     # the reference shape: 12.5 k-chunks, ragged block, xw = 31
    (33, 15, 7, 37, 9, False, None, False),      # scalar loader with a tail, unaligned rows, xw = 32 (column 31 live), a 1-row block
    (1, 11, 3, 1, 1, False, None, False),        # less than one chunk
    (100, 15, 6, 257, 8, False, None, True),     # one column into a ninth chunk: past one chunk per wave; real-valued contacts
    (100, 3, 6, 64, 21, False, None, False),     # the widest embedding that fits
    (80, 15, 6, 400, 8, True, None, False),      # only_contact
    (33, 15, 6, 37, 8, True, None, False),       # only_contact, scalar loader
    (589, 15, 6, 400, 8, False, (64, 8, 2), False),   # rows > mb = 256: the chunk loop
    (8300, 15, 6, 36, 8, False, None, False),    # 260 row blocks x 2 nets: more workgroups than CUs
]


@pytest.mark.parametrize("rows,obs_dim,act,P,E,oc,engine,real", CASES)
def test_fused_contact_step_matches_float64_and_the_layerwise_ops(rows, obs_dim, act, P, E, oc, engine, real):
    """rollout_policy_step_contacts on the persistent kernel: launches (k_policy_stage + k_policy_fwd per chunk of mb rows,
    nothing else), raw arena copies bit for bit, outputs against float64 at the bounds of
    test_rollout_policy_step_off_the_default_widths_matches_float64 and against infer_contacts + rollout_act_store (the
    layer-by-layer launches: k_contact_fwd sums the P terms chunk after chunk on one wave, the persistent kernel as eight
    per-wave partial sums added in wave order) at the bounds test_fused_policy_step_equals_infer_plus_act_store holds the
    kernel without contacts to (2e-6, neglogp 2e-5); and the step is bit-reproducible from call to call."""
    eng, x, d, ref = _setup(rows, obs_dim, act, P, E, oc, engine, real)
    rms_v = torch.tensor(RMS_V, dtype=torch.float64, device="cuda:0")
    a, b, c = (_outs(rows, obs_dim, act, P) for _ in range(3))
    mu, value_n = eng.infer_contacts(d["obs"], d["priv"], d["contacts"], normalize=True)
    torch.ops.mi355ppo.rollout_act_store(d["obs"], d["priv"], mu, value_n, eng.param_views()["sigma"], d["noise"], rms_v, 1e-5,
                                         a["obses"], a["priv"], a["actions"], a["nlp"], a["values"], a["mus"], a["sigmas"],
                                         a["clamped"], a["vout"])
    classes = _classes(lambda: _step(eng, d, b, rms_v))
    chunks = (rows + eng.mb - 1) // eng.mb
    assert classes.get("k_policy_fwd", 0) == chunks and classes.get("other", 0) == chunks, classes
    assert set(classes) == {"k_policy_fwd", "other"}, classes
    # the arena slot: raw copies
    assert torch.equal(b["obses"].cpu(), x["obs"]) and torch.equal(b["priv"].cpu(), x["priv"])
    assert torch.equal(b["contacts"].cpu(), x["contacts"])
    assert torch.equal(b["sigmas"], a["sigmas"])
    want = ref()
    _assert_f64(b, want, "fused ")
    for k in ("mus", "actions", "clamped", "values", "vout"):
        print(f"{k}: max |fused - layerwise| = {float((a[k] - b[k]).abs().max()):.3e}, "
              f"layerwise vs fp64 {np.abs(a[k].cpu().numpy() - want[k].numpy()).max():.3e}")
        np.testing.assert_allclose(b[k].cpu().numpy(), a[k].cpu().numpy(), atol=2e-6, rtol=2e-6, err_msg=k)
    np.testing.assert_allclose(b["nlp"].cpu().numpy(), a["nlp"].cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert float(b["actions"].abs().max()) > 0 and torch.isfinite(b["nlp"]).all()
    # the same inputs again: bit-equal
    _step(eng, d, c, rms_v)
    torch.cuda.synchronize()
    for k in b:
        assert torch.equal(b[k], c[k]), k


def test_a_contact_teacher_outside_the_shape_keeps_the_layerwise_launches():
    """obs 15 + latent 8 + embedding 10 = 33 columns (xld = 64): no persistent kernel, float64 bounds all the same."""
    rows, obs_dim, act, P, E = 80, 15, 6, 400, 10
    eng, x, d, ref = _setup(rows, obs_dim, act, P, E, False)
    rms_v = torch.tensor(RMS_V, dtype=torch.float64, device="cuda:0")
    o = _outs(rows, obs_dim, act, P)
    classes = _classes(lambda: _step(eng, d, o, rms_v))
    assert classes.get("k_policy_fwd", 0) == 0 and classes.get("other", 0) >= 3, classes   # stage, k_contact_fwd, k_heads_act_store
    assert torch.equal(o["contacts"].cpu(), x["contacts"])
    _assert_f64(o, ref())


def test_the_teacher_without_contacts_still_takes_one_persistent_launch():
    rows, obs_dim, act = 80, 15, 6
    eng, x, d, ref = _setup(rows, obs_dim, act, 0, 0, False)
    rms_v = torch.tensor(RMS_V, dtype=torch.float64, device="cuda:0")
    o = _outs(rows, obs_dim, act, 0)
    classes = _classes(lambda: _step(eng, d, o, rms_v))
    assert classes == {"k_policy_fwd": 1, "other": 1}, classes
    _assert_f64(o, ref())


@pytest.mark.parametrize("tag", ["contacts", "only_contact"])
def test_contact_policy_step_matches_reference_at_the_default_network(tag):
    """The reference's own PPO.model_act (ActorCritic.act with contacts, replayed Normal noise) at ITS network shape --
    512 / 256 / 128, 256 / 128 / 8, 400 contact points, embedding 8 -- for 80 environments: the persistent kernel ran, and
    the outputs meet the bounds test_ppo_play_steps_matches_reference holds the same quantities to."""
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    G = np.load(os.path.join(HERE, "golden", "rollout_contacts_default.npz"))
    N, P, E, oc = [int(v) for v in G[f"{tag}/meta"]]
    init = {}
    for k in G[f"{tag}/param_names"]:       # only_contact stores the tensors that differ from the contacts case
        key = f"{tag}/init/{k}" if f"{tag}/init/{k}" in G.files else f"contacts/init/{k}"
        init[str(k)] = torch.from_numpy(G[key].astype(np.float32))
    eng = TeacherEngine(N, 4, 2, units=UNITS, priv_units=PRIV_UNITS, contact_points=P, contact_emb=E, only_contact=bool(oc))
    eng.load_params(init)
    so, sp, sv = (G[f"{tag}/rms_in/{nm}"] for nm in ("running_mean_std", "priv_mean_std", "value_mean_std"))
    eng.rms_obs[:31] = torch.from_numpy(so).cuda()
    eng.rms_priv[:2 * PRIV + 1] = torch.from_numpy(sp).cuda()
    rms_v = torch.from_numpy(sv).cuda()
    d = dict(obs=torch.from_numpy(G[f"{tag}/in/obs"]).cuda(), priv=torch.from_numpy(G[f"{tag}/in/priv_info"]).cuda(),
             contacts=torch.from_numpy(G[f"{tag}/in/contacts"].astype(np.float32)).cuda(),
             noise=torch.from_numpy(G[f"{tag}/in/noise"]).cuda())
    o = _outs(N, 15, 6, P)
    classes = _classes(lambda: _step(eng, d, o, rms_v))
    assert classes == {"k_policy_fwd": 1, "other": 1}, classes
    assert torch.equal(o["contacts"], d["contacts"])
    for k, gk, atol in (("mus", "mus", 2e-5), ("sigmas", "sigmas", 1e-6), ("actions", "actions", 2e-5),
                        ("values", "values", 2e-5), ("nlp", "neglogpacs", 5e-5)):
        want = G[f"{tag}/out/{gk}"]
        got = o[k].cpu().numpy().reshape(want.shape)
        print(f"{k}: max |hip - reference| = {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, atol=atol, rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(o["clamped"].cpu().numpy(), np.clip(G[f"{tag}/out/actions"], -1, 1), atol=2e-5)
    assert (np.abs(G[f"{tag}/out/actions"]) > 1).any()


def test_ppo_play_steps_with_contacts_runs_the_persistent_kernel():
    """PPO at the default network with 400 contact points: one k_policy_fwd per environment step (counted when the
    environment is stepped: the first prepare_training of a trainer re-uses the profiler for its workspace trial), and the
    contacts arena holds what the environment reported, bit for bit."""
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    N, T, P = 64, 4, 400
    # mini_epochs 2: the engine's chunk of mb = N * T / 2 rows holds the N rows of a step (one launch per step)
    cfg = default_config(num_envs=N, horizon_length=T, rl_device="cuda:0", num_points=P, compute_contact_gt=True,
                         mini_epochs=2)
    cfg.task.env.compute_contact_gt = True
    cfg.train.network.contact_mlp.units = [8]
    env = SyntheticInsertionEnv(N, device="cuda:0", contact_points=P)
    agent = PPO(env, None, cfg)
    assert agent.engine.mb >= N
    seen, launches, step = [], [], env.step

    def record(actions):
        torch.cuda.synchronize()
        launches.append(sum(c["launches"] for c in _lib.prof_read() if c["name"].split(":")[0] == "k_policy_fwd"))
        r = step(actions)
        seen.append(r[0]["contacts"].clone())
        return r
    env.step = record
    agent.obs = env.reset()
    first = agent.obs["contacts"].clone()
    agent.set_eval()
    _lib.prof_enable(True)
    try:
        agent.play_steps()
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    stored = agent.storage.storage_dict["contacts"]
    assert stored.shape == (T, N, P) and stored.sum() > 0
    assert torch.equal(stored[0], first)
    for t in range(1, T):
        assert torch.equal(stored[t], seen[t - 1]), t
    assert launches == list(range(1, T + 1)), launches
