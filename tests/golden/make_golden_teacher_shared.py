"""Generate golden vectors of the teacher with a SHARED actor-critic trunk from the REFERENCE implementation.

Runs ONLY in the build container (needs /root/reference).  Follows make_golden_teacher_contacts.py: the reference's own
``algo.ppo.frozen_ppo.PPO`` on CPU (``ref_harness``) with ``cfg.train.ppo.shared_parameters = True`` set on the
returned config (ref_harness.py itself is not edited), its ``ExperienceBuffer`` filled with a seeded synthetic rollout
through its own ``model_act``, then its unmodified ``PPO.train_epoch``.  The model then has no ``critic_mlp``
(models_split.py:100-102) and the value head reads the actor trunk's output (:226-230): 17 state_dict tensors.

Outputs ``teacher_shared_small.npz`` and ``teacher_shared_default.npz`` (same keys as teacher_<case>.npz, plus
``u<u>/act/*``: the normaliser state ``model_act`` used; the default case's initial parameters, step-0 gradient and
final parameters live in ``teacher_shared_default.{init,grad,params}.npz`` so that no file exceeds 1 MiB), and ``teacher_shared_ckpt.npz``: the reference's ``PPO.save``
file contents (model state_dict + normaliser states) after one update of the small case, flattened to arrays.

    python tests/golden/make_golden_teacher_shared.py
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
from make_golden_teacher import flat_params, ref_tail, synth_fill  # noqa: E402


def run_case(name, num_envs, horizon, mini_epochs, units, priv_units, n_updates, done_p, seed=42, data_seed=1234,
             ckpt=False, split=False):
    cfg = rh.teacher_config(num_envs, horizon, mini_epochs, units=units, priv_units=priv_units)
    cfg.train.ppo.shared_parameters = True
    torch.manual_seed(seed)
    agent = PPO(None, None, cfg)
    assert not any(k.startswith("critic_mlp") for k in agent.model.state_dict())
    gen = torch.Generator().manual_seed(data_seed)
    out = {}
    out["meta"] = np.array([num_envs, horizon, mini_epochs, n_updates], dtype=np.int64)
    out["units"] = np.array(units, dtype=np.int64)
    out["priv_units"] = np.array(priv_units, dtype=np.int64)
    for k, v in agent.model.state_dict().items():
        out[f"init/{k}"] = v.numpy().copy()
    out["perm"] = agent.storage.indices.numpy().copy()

    for u in range(n_updates):
        rec = {"grads": [], "norms": []}

        def fake_play_steps(u=u):
            last_values = synth_fill(agent, gen, done_p)
            for k in ["obses", "priv_info", "rewards", "values", "neglogpacs", "dones", "actions", "mus", "sigmas"]:
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
            if len(rec["grads"]) < 1:   # raw (pre-clip) gradient of the first optimizer step
                rec["grads"].append(torch.cat([p.grad.reshape(-1) for p in params]).numpy().copy())
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

        if ckpt and u == 0:   # the reference's own checkpoint writer (frozen_ppo.py save) after one update
            with tempfile.TemporaryDirectory() as d:
                agent.save(os.path.join(d, "ckpt"))
                sd = torch.load(os.path.join(d, "ckpt.pth"), map_location="cpu", weights_only=False)
            flat = {}
            for top, v in sd.items():
                if isinstance(v, dict):
                    for k, t in v.items():
                        if torch.is_tensor(t):
                            flat[f"{top}/{k}"] = t.numpy().copy()
            cpath = os.path.join(HERE, "teacher_shared_ckpt.npz")
            np.savez_compressed(cpath, units=out["units"], priv_units=out["priv_units"], **flat)
            print(f"wrote {cpath}: {os.path.getsize(cpath) / 1e6:.2f} MB, {len(flat)} arrays")

    # a committed fixture stays under 1 MiB: the three parameter-sized groups of the default widths (227,989 floats each)
    # go to companion files teacher_shared_<name>.<part>.npz, which tests/shared_critic_ref.py merges back on load
    parts = {}
    if split:
        for part, pick in (("init", lambda k: k.startswith("init/")), ("grad", lambda k: k.endswith("/grad_step0")),
                           ("params", lambda k: k.endswith("/params_after"))):
            parts[part] = {k: out.pop(k) for k in [k for k in out if pick(k)]}
    for part, arrays in [("", out)] + sorted(parts.items()):
        path = os.path.join(HERE, f"teacher_shared_{name}{'.' + part if part else ''}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), path
        print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")
    print(f"a_loss[0]={out['u0/a_losses'][0]:.6f} c_loss[0]={out['u0/c_losses'][0]:.6f}")


if __name__ == "__main__":
    torch.set_num_threads(1)  # fixed reduction order for reproducible goldens
    run_case("small", num_envs=32, horizon=8, mini_epochs=4, units=(64, 48, 32), priv_units=(48, 32, 8),
             n_updates=2, done_p=0.05, ckpt=True)
    run_case("default", num_envs=64, horizon=8, mini_epochs=4, units=(512, 256, 128), priv_units=(256, 128, 8),
             n_updates=1, done_p=0.05, split=True)
