"""Policy-step golden vectors of the contact teacher at the DEFAULT network, from the REFERENCE implementation (build
container only).

Runs the reference's own ``PPO.model_act`` (frozen_ppo.py:343-366 -> ``ActorCritic.act``, models_split.py:120-183) on CPU
with ``compute_contact_gt``: mlp 512 / 256 / 128, priv_mlp 256 / 128 / 8, num_points 400, contact_mlp.units[-1] = 8, for
N = 80 environments (two whole 32-row blocks of the persistent policy kernel and a ragged 16-row one), in two cases:
contacts and only_contact.  The Gaussian noise of ``Normal.sample`` is replaced by a pre-drawn tensor
(make_golden_rollout.FixedNoise) so that the HIP path can replay the draw.

The reference initialises every bias with zeros and the mu head with std 0.01, which would leave the heads almost
untested: as teacher_case / student_case of make_golden_rollout.py do, the normaliser states, ``sigma`` and the biases
are set to non-trivial values and the mu weights are scaled by 30.  Every parameter is then rounded to a multiple of
1 / 1024 (and kept below 2 in magnitude), which float16 holds exactly: the file stores the parameters as float16 at half
the size, and the test reads back exactly the float32 values the reference computed with.  The only_contact case copies
every tensor whose shape it shares with the contacts case and stores only the others (the first trunk layers).

    python tests/golden/make_golden_rollout_contacts.py  ->  tests/golden/rollout_contacts_default.npz
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
from make_golden_rollout import FixedNoise, set_rms  # noqa: E402

N, P, E = 80, 400, 8
UNITS, PRIV_UNITS = (512, 256, 128), (256, 128, 8)
GRID = 1024.0


def rms_state(m):
    return np.concatenate([m.running_mean.numpy().reshape(-1), m.running_var.numpy().reshape(-1),
                           np.array([m.count.item()])]).astype(np.float64)


def case(out, tag, only_contact, seed, share=None):
    cfg = rh.teacher_config(N, 4, 2, units=UNITS, priv_units=PRIV_UNITS)
    cfg.task.env.compute_contact_gt = True
    cfg.train.ppo.compute_contact_gt = True
    cfg.train.ppo.only_contact = bool(only_contact)
    cfg.train.ppo.num_points = P
    cfg.train.network.contact_mlp.units = [E]
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 100)
    with tempfile.TemporaryDirectory() as d:
        agent = PPO(None, d, cfg)
    with torch.no_grad():
        agent.model.sigma.copy_(0.2 * torch.randn(6, generator=g))
        agent.model.mu.weight.mul_(30.0)        # std-0.01 init -> actions that reach the +-1 clamp
        for k, v in agent.model.named_parameters():
            if k.endswith("bias"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
        for k, v in agent.model.state_dict().items():
            if share is not None and k in share and share[k].shape == v.shape:
                v.copy_(share[k])
            else:
                v.copy_(torch.clamp(torch.round(v * GRID) / GRID, -2.0 + 1.0 / GRID, 2.0 - 1.0 / GRID))
    sd = {k: v.clone() for k, v in agent.model.state_dict().items()}
    for m in (agent.running_mean_std, agent.priv_mean_std, agent.value_mean_std):
        set_rms(m, g)
    out[f"{tag}/meta"] = np.array([N, P, E, int(only_contact)], dtype=np.int64)
    out[f"{tag}/param_names"] = np.array(list(sd.keys()))
    stored = 0
    for k, v in sd.items():
        h = v.to(torch.float16)
        assert torch.equal(h.float(), v), k                # float16 holds the rounded parameters exactly
        if share is None or k not in share or not torch.equal(share[k], v):
            out[f"{tag}/init/{k}"] = h.numpy().copy()
            stored += 1
    for nm in ("running_mean_std", "priv_mean_std", "value_mean_std"):
        out[f"{tag}/rms_in/{nm}"] = rms_state(getattr(agent, nm))
    obs = {"obs": 1.5 * torch.randn(N, 15, generator=g) + 0.2, "priv_info": torch.randn(N, 64, generator=g),
           "contacts": (torch.rand(N, P, generator=g) < 0.2).float()}
    noise = torch.randn(1, N, 6, generator=g)
    for k, v in obs.items():
        out[f"{tag}/in/{k}"] = (v.to(torch.uint8) if k == "contacts" else v).numpy().copy()
    out[f"{tag}/in/noise"] = noise[0].numpy().copy()
    agent.set_eval()
    with torch.no_grad(), FixedNoise(noise):
        res = agent.model_act(obs)
    for k in ("actions", "neglogpacs", "values", "mus", "sigmas"):
        out[f"{tag}/out/{k}"] = res[k].numpy().copy()
    print(tag, f"{stored} of {len(sd)} tensors stored; clamped fraction",
          float((res["actions"].abs() > 1).float().mean()), "mu std", float(res["mus"].std()),
          "value std", float(res["values"].std()))
    return sd


if __name__ == "__main__":
    torch.set_num_threads(1)
    out = {}
    sd = case(out, "contacts", False, seed=3)
    case(out, "only_contact", True, seed=4, share=sd)
    path = os.path.join(HERE, "rollout_contacts_default.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")
