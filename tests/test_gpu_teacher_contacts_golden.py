"""The contact teacher against golden vectors captured from the REFERENCE's own PPO (tests/golden/
make_golden_teacher_contacts.py): whole updates at test_teacher_matches_reference_golden's tolerances, the trainer
(PPO + ExperienceBuffer + play_steps on the synthetic env), a checkpoint the reference wrote, save / restore, and the
one-rank RCCL update."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("obses", "priv_info", "rewards", "values", "neglogpacs", "dones", "actions", "mus", "sigmas", "last_values",
        "contacts")


def _load(case):
    z = np.load(os.path.join(GOLDEN, f"teacher_contacts_{case}.npz"))
    g = {k: z[k] for k in z.files}
    N, T, E, n_up = [int(x) for x in g["meta"]]
    P, emb, oc = [int(x) for x in g["meta_contacts"]]
    meta = dict(num_envs=N, horizon=T, mini_epochs=E, n_updates=n_up, P=P, emb=emb, only_contact=bool(oc),
                units=[int(x) for x in g["units"]], priv_units=[int(x) for x in g["priv_units"]])
    init = OrderedDict((k[5:], torch.from_numpy(v)) for k, v in g.items() if k.startswith("init/"))
    return g, meta, init


def _engine(meta, init, perm):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    eng = TeacherEngine(meta["num_envs"], meta["horizon"], meta["mini_epochs"], units=meta["units"],
                        priv_units=meta["priv_units"], perm=perm, contact_points=meta["P"], contact_emb=meta["emb"],
                        only_contact=meta["only_contact"])
    eng.load_params(init)
    return eng


@pytest.mark.parametrize("case", ["contacts", "only_contact"])
def test_contact_teacher_matches_reference_golden(case):
    g, meta, init = _load(case)
    eng = _engine(meta, init, torch.from_numpy(g["perm"]))
    lr = 2.5e-4
    frozen = [k for k in eng.shapes if k.startswith("contact_ae.contact_dec_mlp")
              or (meta["only_contact"] and k.startswith("env_mlp"))]
    for u in range(meta["n_updates"]):
        ro = {k: torch.from_numpy(g[f"u{u}/in/{k}"]).cuda() for k in KEYS}
        eng.prepare(ro)
        torch.cuda.synchronize()
        assert np.array_equal(eng.returns_raw.cpu().numpy(), g[f"u{u}/returns_raw"])
        np.testing.assert_allclose(eng.env_major(eng.advantages).cpu().numpy(), g[f"u{u}/advantages"], atol=2e-5,
                                   rtol=1e-5)
        eng.fwd_bwd(0, 0)
        torch.cuda.synchronize()
        g0 = eng.packed(eng.grads).cpu().numpy()
        ref0 = g[f"u{u}/grad_step0"]
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
        np.testing.assert_allclose(s[:, 6], g[f"u{u}/param_norms"], rtol=1e-5)   # includes the frozen tensors
        np.testing.assert_allclose(eng.packed().cpu().numpy(), g[f"u{u}/params_after"],
                                   atol=n_steps * lr * 0.02 * (u + 1), rtol=0)
        np.testing.assert_allclose(eng.env_major(eng.mus_w).cpu().numpy(), g[f"u{u}/mus_after"], atol=2e-4)
        views, m, v = eng.param_views(), eng.param_views(eng.adam_m), eng.param_views(eng.adam_v)
        for k in frozen:   # grad None in the reference: parameter and Adam moments bit-unchanged
            assert torch.equal(views[k].cpu(), init[k]), k
            assert not m[k].any() and not v[k].any(), k


def _ppo(num_envs, horizon, mini_epochs, P, env=None, out=None, units=(64, 48, 32), priv_units=(48, 32, 8)):
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=num_envs, horizon_length=horizon, rl_device="cuda:0", mini_epochs=mini_epochs,
                         num_points=P, compute_contact_gt=True)
    cfg.task.env.compute_contact_gt = True
    cfg.train.network.mlp.units = list(units)
    cfg.train.network.priv_mlp.units = list(priv_units)
    cfg.train.network.contact_mlp.units = [8]
    return PPO(env, out, cfg)


def test_ppo_play_steps_stores_contacts_and_trains(tmp_path):
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    N, T, P = 64, 8, 37
    env = SyntheticInsertionEnv(N, device="cuda:0", contact_points=P)
    agent = _ppo(N, T, 4, P, env=env, out=str(tmp_path))
    assert agent.engine.contact_points == P and agent.storage.storage_dict["contacts"].shape == (T, N, P)
    seen = []
    step = env.step

    def record(actions):
        r = step(actions)
        seen.append(r[0]["contacts"].clone())
        return r
    env.step = record
    agent.obs = env.reset()
    first = agent.obs["contacts"].clone()
    agent.set_eval()
    agent.play_steps()
    torch.cuda.synchronize()
    stored = agent.storage.storage_dict["contacts"]
    assert torch.equal(stored[0], first)
    for t in range(1, T):
        assert torch.equal(stored[t], seen[t - 1]), t
    assert stored.sum() > 0
    # minibatch view gathers the contacts with the same permutation
    vals, nlp, adv, mus, sig, ret, act, obs, priv, contacts = agent.storage[1]
    b = agent.storage.indices[agent.minibatch_size:2 * agent.minibatch_size]
    assert torch.equal(contacts, stored[b % T, b // T])
    agent.set_train()
    before = agent.engine.params.clone()
    agent.train_epoch()
    torch.cuda.synchronize()
    assert torch.isfinite(agent.engine.params).all() and not torch.equal(before, agent.engine.params)
    # act_inference with contacts: latent_gt = [priv latent | contact embedding]
    mu, latent = agent.model.act_inference({"obs": obs[:10], "priv_info": priv[:10], "contacts": contacts[:10]})
    assert mu.shape == (10, 6) and latent.shape == (10, 16)


def test_reference_checkpoint_loads_and_save_restore_round_trips(tmp_path):
    z = np.load(os.path.join(GOLDEN, "teacher_contacts_ckpt.npz"))
    P = int(z["meta_contacts"][0])
    ck = {}
    for k in z.files:
        if "/" in k:
            top, name = k.split("/", 1)
            ck.setdefault(top, OrderedDict())[name] = torch.from_numpy(z[k])
    path = str(tmp_path / "ref.pth")
    torch.save(ck, path)
    agent = _ppo(32, 8, 4, P, units=[int(x) for x in z["units"]], priv_units=[int(x) for x in z["priv_units"]])
    agent.restore_test(path)
    sd = agent.model.state_dict()
    assert list(sd.keys()) == list(ck["model"].keys())
    for k, v in ck["model"].items():
        assert torch.equal(sd[k].cpu(), v), k
    np.testing.assert_array_equal(agent.running_mean_std.state_dict()["running_mean"].cpu().numpy(),
                                  ck["running_mean_std"]["running_mean"].numpy())
    # the engine sees the restored weights: inference equals a float64 restatement of the reference's forward
    g = torch.Generator().manual_seed(0)
    obs, priv = torch.randn(20, 15, generator=g), torch.randn(20, 64, generator=g)
    cts = (torch.rand(20, P, generator=g) < 0.2).float()
    mu, _ = agent.model.act_inference({"obs": obs.cuda(), "priv_info": priv.cuda(), "contacts": cts.cuda()})
    p = {k: v.double() for k, v in ck["model"].items()}

    def mlp(pre, n, x):
        for i in range(n):
            x = torch.tanh(x @ p[f"{pre}.mlp.{2 * i}.weight"].T + p[f"{pre}.mlp.{2 * i}.bias"])
        return x
    h = torch.relu(cts.double() @ p["contact_ae.contact_enc_mlp.0.weight"].T + p["contact_ae.contact_enc_mlp.0.bias"])
    ec = torch.tanh(h @ p["contact_ae.contact_enc_mlp.2.weight"].T + p["contact_ae.contact_enc_mlp.2.bias"])
    x = torch.cat([obs.double(), mlp("env_mlp", 3, priv.double()), ec], -1)
    mu_ref = mlp("actor_mlp", 3, x) @ p["mu.weight"].T + p["mu.bias"]
    np.testing.assert_allclose(mu.cpu().numpy(), mu_ref.numpy(), atol=1e-5)
    # save / restore round trip through this package
    agent.save(str(tmp_path / "mine"))
    other = _ppo(32, 8, 4, P, units=[int(x) for x in z["units"]], priv_units=[int(x) for x in z["priv_units"]])
    other.restore_train(str(tmp_path / "mine.pth"))
    assert torch.equal(other.engine.params, agent.engine.params)


def test_contact_native_rccl_update_on_a_one_rank_communicator():
    from isaacgyminsertion_amd.utils.dist import NativeComm
    g, meta, init = _load("contacts")
    torch.cuda.set_device(0)
    comm = NativeComm(rank=0, world=1)
    ro = {k: torch.from_numpy(g[f"u0/in/{k}"]).cuda() for k in KEYS}

    def run(mode):
        eng = _engine(meta, init, torch.from_numpy(g["perm"]))
        eng.prepare(ro)
        if mode == "single":
            eng.update()
        else:
            eng.update_dp_native(comm, overlap=(mode == "overlap"))
        torch.cuda.synchronize()
        return eng.params.clone(), eng.stats.clone(), eng.adam_m.clone(), eng.adam_v.clone()

    ref = run("single")
    for mode in ("overlap", "serial"):
        got = run(mode)
        for a, b in zip(ref, got):
            assert torch.equal(a, b), mode
    comm.close()
