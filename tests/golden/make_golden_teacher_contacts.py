"""Generate golden vectors of the teacher WITH ground-truth contacts from the REFERENCE implementation.

Runs ONLY in the build container (needs /root/reference).  Follows make_golden_teacher.py: the reference's own
``algo.ppo.frozen_ppo.PPO`` on CPU (``ref_harness``), its ``ExperienceBuffer`` filled with a seeded synthetic
rollout through its own ``model_act`` -- here with 0/1 ``contacts`` in the observation, stored per step as
play_steps does (frozen_ppo.py:655-683) -- then its unmodified ``PPO.train_epoch``.  The contact flags are set by
overriding the returned config (task.env / train.ppo ``compute_contact_gt``, ``only_contact``, ``num_points``,
``train.network.contact_mlp.units``); ref_harness.py itself is not edited.

Parameters without a gradient (the ContactAE decoder always, env_mlp under only_contact) have ``grad = None`` in
the reference: the recording ``clip_grad_norm_`` hook writes zeros in their slots of the flat gradient.

Outputs ``teacher_contacts_<case>.npz`` (same keys as teacher_<case>.npz, plus ``u<u>/in/contacts`` and
``meta_contacts`` = [P, E, only_contact]), and ``teacher_contacts_ckpt.npz``: the reference's ``PPO.save`` file
contents (model state_dict + normaliser states) after one update, flattened to arrays.

    python tests/golden/make_golden_teacher_contacts.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.install()
from algo.ppo.frozen_ppo import PPO  # noqa: E402  (reference)
from make_golden_teacher import flat_params, ref_tail  # noqa: E402


def contact_config(num_envs, horizon, mini_epochs, units, priv_units, P, E, only_contact):
    cfg = rh.teacher_config(num_envs, horizon, mini_epochs, units=units, priv_units=priv_units)
    cfg.task.env.compute_contact_gt = True
    cfg.train.ppo.compute_contact_gt = True
    cfg.train.ppo.only_contact = bool(only_contact)
    cfg.train.ppo.num_points = P
    cfg.train.network.contact_mlp.units = [E]
    return cfg


def synth_fill(agent, gen, done_p, P):
    """What play_steps stores (frozen_ppo.py:655-683) for a synthetic env that also reports contacts."""
    st = agent.storage
    T, N = st.transitions_per_env, st.num_envs
    obs_dim, priv_dim = st.obs_dim, st.priv_dim

    def draw():
        return {"obs": torch.randn(N, obs_dim, generator=gen),
                "priv_info": torch.randn(N, priv_dim, generator=gen),
                "contacts": (torch.rand(N, P, generator=gen) < 0.2).float()}

    for n in range(T):
        obs = draw()
        res = agent.model_act(obs)
        st.update_data("obses", n, obs["obs"])
        st.update_data("priv_info", n, obs["priv_info"])
        st.update_data("contacts", n, obs["contacts"])
        for k in ["actions", "neglogpacs", "values", "mus", "sigmas"]:
            st.update_data(k, n, res[k])
        dones = (torch.rand(N, generator=gen) < done_p).to(torch.uint8)
        st.update_data("dones", n, dones)
        st.update_data("rewards", n, 0.1 * torch.randn(N, 1, generator=gen))
    return agent.model_act(draw())["values"]


def run_case(name, num_envs, horizon, mini_epochs, units, priv_units, P, E, only_contact, n_updates, done_p,
             seed=42, data_seed=1234, ckpt=False):
    cfg = contact_config(num_envs, horizon, mini_epochs, units, priv_units, P, E, only_contact)
    torch.manual_seed(seed)
    agent = PPO(None, None, cfg)
    gen = torch.Generator().manual_seed(data_seed)
    out = {}
    out["meta"] = np.array([num_envs, horizon, mini_epochs, n_updates], dtype=np.int64)
    out["meta_contacts"] = np.array([P, E, int(only_contact)], dtype=np.int64)
    out["units"] = np.array(units, dtype=np.int64)
    out["priv_units"] = np.array(priv_units, dtype=np.int64)
    for k, v in agent.model.state_dict().items():
        out[f"init/{k}"] = v.numpy().copy()
    out["perm"] = agent.storage.indices.numpy().copy()

    for u in range(n_updates):
        rec = {"grads": [], "norms": []}

        def fake_play_steps(u=u):
            last_values = synth_fill(agent, gen, done_p, P)
            for k in ["obses", "priv_info", "contacts", "rewards", "values", "neglogpacs", "dones", "actions",
                      "mus", "sigmas"]:
                out[f"u{u}/in/{k}"] = agent.storage.storage_dict[k].numpy().copy()
            out[f"u{u}/in/last_values"] = last_values.numpy().copy()
            for nm in ["running_mean_std", "priv_mean_std"]:        # the state model_act normalised with
                m = getattr(agent, nm)
                out[f"u{u}/act/{nm}/running_mean"] = m.running_mean.numpy().copy()
                out[f"u{u}/act/{nm}/running_var"] = m.running_var.numpy().copy()
                out[f"u{u}/act/{nm}/count"] = np.array(m.count.item(), dtype=np.float64)
            ref_tail(agent, last_values)
            dd = agent.storage.data_dict
            out[f"u{u}/returns_raw"] = agent.storage.storage_dict["returns"].numpy().copy()
            out[f"u{u}/advantages"] = dd["advantages"].numpy().copy()
            out[f"u{u}/values_norm"] = dd["values"].numpy().copy()
            out[f"u{u}/returns_norm"] = dd["returns"].numpy().copy()
            out[f"u{u}/vms_after_tail"] = np.array(
                [agent.value_mean_std.running_mean.item(), agent.value_mean_std.running_var.item(),
                 agent.value_mean_std.count.item()], dtype=np.float64)

        agent.play_steps = fake_play_steps
        orig_clip = torch.nn.utils.clip_grad_norm_

        def rec_clip(params, max_norm, *a, **k):
            params = list(params)
            if len(rec["grads"]) < 2:   # raw gradient, zeros where grad is None (decoder; env_mlp with only_contact)
                rec["grads"].append(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                                               for p in params]).numpy().copy())
            n = orig_clip(params, max_norm, *a, **k)
            rec["norms"].append(float(n))
            return n

        torch.nn.utils.clip_grad_norm_ = rec_clip
        try:
            a_losses, c_losses, b_losses, entropies, kls, grad_norms, _ = agent.train_epoch()
        finally:
            torch.nn.utils.clip_grad_norm_ = orig_clip

        out[f"u{u}/a_losses"] = np.array([x.item() for x in a_losses], dtype=np.float32)
        out[f"u{u}/c_losses"] = np.array([x.item() for x in c_losses], dtype=np.float32)
        out[f"u{u}/b_losses"] = np.array([x.item() for x in b_losses], dtype=np.float32)
        out[f"u{u}/entropies"] = np.array([x.item() for x in entropies], dtype=np.float32)
        out[f"u{u}/kls"] = np.array([x.item() for x in kls], dtype=np.float32)
        out[f"u{u}/param_norms"] = np.array([x.item() for x in grad_norms], dtype=np.float32)
        out[f"u{u}/grad_total_norms"] = np.array(rec["norms"], dtype=np.float32)
        out[f"u{u}/grad_step0"] = rec["grads"][0]
        out[f"u{u}/params_after"] = flat_params(agent.model)
        out[f"u{u}/mus_after"] = agent.storage.data_dict["mus"].numpy().copy()
        out[f"u{u}/sigmas_after"] = agent.storage.data_dict["sigmas"].numpy().copy()
        for nm in ["running_mean_std", "priv_mean_std", "value_mean_std"]:
            m = getattr(agent, nm)
            out[f"u{u}/{nm}/running_mean"] = m.running_mean.numpy().copy()
            out[f"u{u}/{nm}/running_var"] = m.running_var.numpy().copy()
            out[f"u{u}/{nm}/count"] = np.array(m.count.item(), dtype=np.float64)

    path = os.path.join(HERE, f"teacher_contacts_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB, a_loss[0]={out['u0/a_losses'][0]:.6f}")

    if ckpt:   # the reference's own checkpoint writer (frozen_ppo.py save)
        with tempfile.TemporaryDirectory() as d:
            agent.save(os.path.join(d, "ckpt"))
            sd = torch.load(os.path.join(d, "ckpt.pth"), map_location="cpu", weights_only=False)
        flat = {}
        for top, v in sd.items():
            if isinstance(v, dict):
                for k, t in v.items():
                    if torch.is_tensor(t):
                        flat[f"{top}/{k}"] = t.numpy().copy()
        cpath = os.path.join(HERE, f"teacher_contacts_ckpt.npz")
        np.savez_compressed(cpath, meta_contacts=out["meta_contacts"], units=out["units"],
                            priv_units=out["priv_units"], **flat)
        print(f"wrote {cpath}: {os.path.getsize(cpath) / 1e6:.2f} MB, {len(flat)} arrays")


if __name__ == "__main__":
    torch.set_num_threads(1)  # fixed reduction order for reproducible goldens
    run_case("contacts", num_envs=32, horizon=8, mini_epochs=4, units=(64, 48, 32), priv_units=(48, 32, 8),
             P=37, E=8, only_contact=False, n_updates=2, done_p=0.05, ckpt=True)
    run_case("only_contact", num_envs=32, horizon=8, mini_epochs=4, units=(64, 48, 32), priv_units=(48, 32, 8),
             P=37, E=8, only_contact=True, n_updates=1, done_p=0.05)
