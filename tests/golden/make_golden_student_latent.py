"""Golden vectors of the LATENT student (offline_train.only_bc=False) with the latent term of the loss live, from the
REFERENCE implementation (build container only).

Builds the reference's own ``ExtrinsicAdapt`` exactly as ``make_golden_student.py`` does (stand-in env, xavier student
weights, ``mu.weight`` of the frozen teacher scaled to O(1) actions, a seeded synthetic rollout in the reference's
``StudentBuffer``), lin-only student, 20 envs x 7 steps x 2 mini-epochs: minibatches of 70 rows = two full 32-row blocks
and a ragged one.  For minibatch 0 it executes the statements of the reference's ``train_epoch`` (ext_adapt.py:785-828) on
the reference's own modules -- ``student.predict``, ``agent.act_with_grad``, ``torch.nn.MSELoss`` -- with line 827 as it
reads once its comment sign is removed,

    loss = (self.action_scale * loss_action) + (self.latent_scale * loss_latent)

at (action_scale, latent_scale) = (1, 0), (1, 1), (1.3, 0.7), and stores the inputs and the permutation, both
state_dicts, ``mu``, ``latent``, d loss / d latent, both losses and the gradient of every student parameter, plus the
distance of each gradient tensor to the same statements rerun in float64 (``grad0_ref_noise``).  The teacher's seven weight
matrices above 10 000 entries would take the fixture past its size limit: they are seeded stand-ins (``big_weight`` of
make_golden_student.py, as for the depth backbone there) that the tests regenerate; every other tensor is stored.

    python tests/golden/make_golden_student_latent.py  ->  tests/golden/student_latent.npz
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_student as mgs  # noqa: E402  (installs the reference import harness)
from algo.ext_adapt.ext_adapt import ExtrinsicAdapt  # noqa: E402  (reference)

TAG = "lin_latent70"
N, T, E, SEED = 20, 7, 2, 13
SCALES = ((1.0, 0.0), (1.0, 1.0), (1.3, 0.7))
BIG_TEACHER = 10_000    # teacher tensors above this size are seeded stand-ins, not stored


def build_agent():
    cfg = mgs.student_config(N, T, E, False, False, False)
    cfg.offline_train.only_bc = False
    env = mgs.FakeEnv(N, False, False, False)
    torch.manual_seed(SEED)
    orig_to = torch.nn.Module.to
    torch.nn.Module.to = lambda self, *a, **k: self
    try:
        with tempfile.TemporaryDirectory() as d:
            agent = ExtrinsicAdapt(env, d, cfg)
    finally:
        torch.nn.Module.to = orig_to
    agent.student.device = "cpu"
    model = agent.student.model
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight, generator=g)
                m.bias.uniform_(-0.1, 0.1, generator=g)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    tg = torch.Generator().manual_seed(SEED + 7)
    with torch.no_grad():
        agent.agent.mu.weight.copy_(torch.randn(agent.agent.mu.weight.shape, generator=tg) * 0.3)
        for k, v in agent.agent.state_dict().items():
            if v.numel() > BIG_TEACHER:
                v.copy_(mgs.big_weight(k, v.shape, SEED))
    st = agent.storage
    for t in range(T):
        st.update_data('n_obs', t, torch.randn(N, 15, generator=g))
        st.update_data('n_priv_info', t, torch.randn(N, 64, generator=g))
        st.update_data('latent_gt', t, torch.randn(N, 8, generator=g))
        st.update_data('teacher_actions', t, torch.rand(N, 6, generator=g) * 2.4 - 1.2)
        st.update_data('student_actions', t, torch.rand(N, 6, generator=g) * 2.4 - 1.2)
        st.update_data('n_student_obs', t, torch.randn(N, 15, generator=g))
    st.prepare_training()
    return agent


def step0(agent, action_scale, latent_scale):
    """ext_adapt.py:785-828 for minibatch 0, the latent term of line 827 live."""
    self = agent
    self.action_scale, self.latent_scale = action_scale, latent_scale
    self.set_student_train()
    loss_latent_fn = torch.nn.MSELoss()
    batched_obs = self.storage[0]
    student_dict = {'student_obs': batched_obs['n_student_obs'], 'tactile': None, 'img': None, 'seg': None, 'pcl': None}
    latent, _ = self.student.predict(student_dict, requires_grad=True)
    latent.retain_grad()
    mu, _ = self.agent.act_with_grad({'obs': batched_obs['n_obs'], 'latent': latent})
    loss_latent = loss_latent_fn(latent, batched_obs['latent_gt'].detach())
    weights = torch.ones(6, device=self.device)
    weights[2] = 0.1
    loss_action = (torch.clamp(mu, -1, 1) - torch.clamp(batched_obs['teacher_actions'].detach(), -1, 1)) ** 2
    loss_action = torch.sum(loss_action * weights.to(loss_action.dtype)).mean()
    self.optim.zero_grad()
    loss = (self.action_scale * loss_action) + (self.latent_scale * loss_latent)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in self.student.model.named_parameters() if p.grad is not None}
    return dict(mu=mu.detach().clone(), latent=latent.detach().clone(), dlatent=latent.grad.detach().clone(),
                loss_action=loss_action.detach().clone(), loss_latent=loss_latent.detach().clone(), grads=grads)


if __name__ == "__main__":
    torch.set_num_threads(1)
    agent = build_agent()
    agent64 = copy.deepcopy(agent)
    agent64.student.model.double()
    agent64.agent.double()
    for k, v in agent64.storage.data_dict.items():
        if v.is_floating_point():
            agent64.storage.data_dict[k] = v.double()
    out = {f"{TAG}/flags": np.array([N, T, E, 0, 0, 0], dtype=np.int64),
           f"{TAG}/scales": np.array(SCALES, dtype=np.float64),
           f"{TAG}/keys": np.array(list(agent.student.model.state_dict().keys())),
           f"{TAG}/perm": agent.storage.indices.numpy().copy()}
    for k, v in agent.student.model.state_dict().items():
        out[f"{TAG}/init/{k}"] = v.numpy().copy()
    out[f"{TAG}/teacher_keys"] = np.array(list(agent.agent.state_dict().keys()))
    for k, v in agent.agent.state_dict().items():
        if v.numel() <= BIG_TEACHER:
            out[f"{TAG}/teacher/{k}"] = v.numpy().copy()
    for k in ('n_obs', 'latent_gt', 'teacher_actions', 'n_student_obs'):    # what the latent student's update reads
        out[f"{TAG}/in/{k}"] = agent.storage.storage_dict[k].numpy().copy()
    for c, (a_s, l_s) in enumerate(SCALES):
        r, r64 = step0(agent, a_s, l_s), step0(agent64, a_s, l_s)
        for k in ("mu", "latent", "dlatent", "loss_action", "loss_latent"):
            out[f"{TAG}/case{c}/{k}"] = r[k].numpy().copy()
            out[f"{TAG}/case{c}/{k}_ref_noise"] = np.array((r[k].double() - r64[k]).abs().max().item(), dtype=np.float64)
        for n, g in r["grads"].items():
            out[f"{TAG}/case{c}/grad0/{n}"] = g.numpy().copy()
            out[f"{TAG}/case{c}/grad0_ref_noise/{n}"] = np.array((g.double() - r64["grads"][n]).abs().max().item(),
                                                                 dtype=np.float64)
        print(f"case {c}: scales {a_s}, {l_s}: loss_action {float(r['loss_action']):.6f} loss_latent "
              f"{float(r['loss_latent']):.6f}, {len(r['grads'])} gradient tensors")
    path = os.path.join(HERE, "student_latent.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")
