"""Reference of the LATENT student's step (offline_train.only_bc=False; ext_adapt.py:785-828 with the latent term of line
827 live), for tests/test_latent_student_cpu.py, tests/test_gpu_actor_latent.py and tests/test_gpu_latent_loss.py.  A
restatement in plain torch, any dtype, around the oracle's own code (oracle/student.py, oracle/teacher.py, not edited):

    latent = oracle.student.forward(sd, student_obs=..., only_bc=False)
    mu     = linear(oracle.teacher._tanh_mlp(teacher, "actor_mlp", n_layers, cat(n_obs, latent)), mu.weight, mu.bias)
    loss   = action_scale * oracle.student.bc_loss(mu, a) + latent_scale * mse(latent, latent_gt)

with the gradients by autograd.  Pinned to goldens captured from the reference's own modules (student.npz: lin_latent;
student_latent.npz) by test_latent_student_cpu.py.  Nothing here needs a GPU."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import student as os_, teacher as ot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAG = "lin_latent70"
BIG_TEACHER = 10_000


def big_weight(name, shape, seed):
    """tests/golden/make_golden_student.py:big_weight -- the seeded stand-in of a tensor the fixture does not store."""
    g = torch.Generator().manual_seed(seed * 1000 + sum(ord(c) for c in name))
    return torch.randn(shape, generator=g) * (1.0 / shape[-1] ** 0.5)


def n_layers(teacher, prefix="actor_mlp"):
    return len([k for k in teacher if k.startswith(prefix + ".mlp.") and k.endswith(".weight")])


def actor_activations(teacher, obs, latent):
    """[h_1, ..., h_nl] of the frozen actor on cat(obs, latent): tanh after every layer (models_split.py:31-35)."""
    hs, x = [], torch.cat([obs, latent], dim=-1)
    for i in range(n_layers(teacher)):
        x = ot._tanh_mlp({"m.mlp.0.weight": teacher[f"actor_mlp.mlp.{2 * i}.weight"],
                          "m.mlp.0.bias": teacher[f"actor_mlp.mlp.{2 * i}.bias"]}, "m", 1, x)
        hs.append(x)
    return hs


def actor_mu(teacher, obs, latent):
    """models_split.py:187-216 with a student latent, the policy head only."""
    h = ot._tanh_mlp(teacher, "actor_mlp", n_layers(teacher), torch.cat([obs, latent], dim=-1))
    return F.linear(h, teacher["mu.weight"], teacher["mu.bias"])


def step(sd, teacher, student_obs, n_obs, actions, latent_gt, action_scale, latent_scale, dtype=torch.float64):
    """One minibatch of the latent student: dict(mu, latent, dlatent, loss_action, loss_latent, grads) in ``dtype``."""
    c = lambda t: t.detach().cpu().to(dtype)   # noqa: E731
    sd = {k: c(v).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    teacher = {k: c(v) for k, v in teacher.items()}
    latent = os_.forward(sd, student_obs=c(student_obs), only_bc=False)
    latent.retain_grad()
    mu = actor_mu(teacher, c(n_obs), latent)
    loss_action = os_.bc_loss(mu, c(actions))
    loss_latent = F.mse_loss(latent, c(latent_gt))
    (action_scale * loss_action + latent_scale * loss_latent).backward()
    return dict(mu=mu.detach(), latent=latent.detach(), dlatent=latent.grad.detach(), loss_action=loss_action.detach(),
                loss_latent=loss_latent.detach(), grads={k: v.grad for k, v in sd.items() if v.grad is not None})


def minibatch0(G, tag, keys=("n_student_obs", "n_obs", "teacher_actions", "latent_gt")):
    """Rows of minibatch 0 of a golden case: sample id b = n * T + t lives at arena[t, n] (experience.py:39-46)."""
    N, T, E = [int(v) for v in G[f"{tag}/flags"][:3]]
    ids = torch.from_numpy(G[f"{tag}/perm"]).long()[: N * T // E]
    t, n = ids % T, ids // T
    return [torch.from_numpy(G[f"{tag}/in/{k}"])[t, n].reshape(len(ids), -1) for k in keys]


def load_latent_golden():
    """(G, student state_dict, teacher state_dict) of tests/golden/student_latent.npz, the seeded stand-ins regenerated."""
    G = np.load(os.path.join(GOLDEN, "student_latent.npz"))
    sd = {k[len(TAG) + 6:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{TAG}/init/")}
    shapes = ot.teacher_param_shapes(15, 64, 6, [512, 256, 128], [256, 128, 8])
    teacher = {}
    for k in [str(x) for x in G[f"{TAG}/teacher_keys"]]:
        stored = f"{TAG}/teacher/{k}"
        teacher[k] = torch.from_numpy(G[stored]) if stored in G.files else big_weight(k, tuple(shapes[k]), 13)
    return G, sd, teacher
