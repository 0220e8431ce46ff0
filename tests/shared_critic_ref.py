"""Reference of the teacher with a SHARED actor-critic trunk (train.ppo.shared_parameters: no critic_mlp, value =
value(actor_mlp(x)); models_split.py:100-102, 226-230), for tests/test_shared_critic_cpu.py and
tests/test_gpu_shared_critic.py.  A restatement in plain torch (any dtype: fp32 for the update, float64 for inference)
around the oracle's own normaliser, GAE, gather, loss, clip_grad_norm_ and torch.optim.Adam code (oracle/teacher.py, which
has no shared mode and is not edited): ``SharedTeacherOracle`` is ``TeacherOracle`` whose forward is ``forward_train``
below.  Pinned to goldens captured from the reference itself (tests/golden/make_golden_teacher_shared.py) by
test_shared_critic_cpu.py.  Nothing here needs a GPU."""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import synth, teacher as ot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARTS = ("init", "grad", "params")   # companion files of a case whose parameter-sized arrays would pass 1 MiB


def param_shapes(obs_dim, priv_dim, act_dim, units, priv_units):
    """state_dict order with shared_parameters: the separate-critic order minus critic_mlp.*."""
    full = ot.teacher_param_shapes(obs_dim, priv_dim, act_dim, units, priv_units)
    return OrderedDict((k, v) for k, v in full.items() if not k.startswith("critic_mlp"))


def actor_critic(p, obs, priv, n_priv_layers, n_layers):
    """models_split.py:166-232 with shared_parameters: ONE trunk, both heads on its output."""
    extrin_gt = ot._tanh_mlp(p, "env_mlp", n_priv_layers, priv)
    x = ot._tanh_mlp(p, "actor_mlp", n_layers, torch.cat([obs, extrin_gt], dim=-1))
    mu = torch.nn.functional.linear(x, p["mu.weight"], p["mu.bias"])
    logstd = mu * 0 + p["sigma"]
    value = torch.nn.functional.linear(x, p["value.weight"], p["value.bias"])
    return mu, logstd, value, extrin_gt


def forward_train(p, obs, priv, prev_actions, n_priv_layers, n_layers):
    """ActorCriticSplit.forward (models_split.py:234-250) on the shared trunk."""
    mu, logstd, value, _ = actor_critic(p, obs, priv, n_priv_layers, n_layers)
    sigma = torch.exp(logstd)
    distr = torch.distributions.Normal(mu, sigma)
    return -distr.log_prob(prev_actions).sum(1), value, distr.entropy().sum(dim=-1), mu, sigma


class SharedTeacherOracle(ot.TeacherOracle):
    """The oracle's update loop driven with the shared forward: update() looks ``forward_train`` up in oracle.teacher at
    call time, so it is swapped for the duration of the call and put back."""

    def __init__(self, params, *a, **k):
        assert not any(n.startswith("critic_mlp") for n in params)
        super().__init__(params, *a, **k)

    def update(self, *a, **k):
        keep = ot.forward_train
        ot.forward_train = forward_train
        try:
            return super().update(*a, **k)
        finally:
            ot.forward_train = keep


def problem(N, T, units, priv_units, obs_dim=15, act_dim=6, seed=1234, done_p=0.05):
    """synth.teacher_problem without critic_mlp, value head re-pointed at the actor trunk: the rollout's old values are
    recomputed with THAT network (the old policy is the initial network; mus / sigmas / actions / neglogpacs do not
    depend on the critic and stay)."""
    base, ro, perm = synth.teacher_problem(N, T, units, priv_units, obs_dim=obs_dim, act_dim=act_dim, seed=seed,
                                           done_p=done_p)
    init = OrderedDict((k, v.clone().float()) for k, v in base.items() if not k.startswith("critic_mlp"))
    assert list(init) == list(param_shapes(obs_dim, 64, act_dim, units, priv_units))
    ro = dict(ro)
    rs_o, rs_p, rs_v = ot.RmsState(obs_dim), ot.RmsState(64), ot.RmsState(1)
    with torch.no_grad():
        def values(o, q):
            _, _, v, _ = actor_critic(init, rs_o.normalize(o), rs_p.normalize(q), len(priv_units), len(units))
            return rs_v.unnormalize(v)
        ro["values"] = values(ro["obses"].reshape(-1, obs_dim), ro["priv_info"].reshape(-1, 64)).reshape(T, N, 1).contiguous()
        g = torch.Generator().manual_seed(seed + 7)
        ro["last_values"] = values(torch.randn(N, obs_dim, generator=g), torch.randn(N, 64, generator=g)).contiguous()
    return init, ro, perm


def load(case):
    """teacher_shared_<case>.npz (+ its companion part files) as golden_io.load_teacher returns a case."""
    g = {}
    for part in ("",) + PARTS:
        path = os.path.join(GOLDEN, f"teacher_shared_{case}{'.' + part if part else ''}.npz")
        if part and not os.path.exists(path):
            continue
        z = np.load(path)
        g.update({k: z[k] for k in z.files})
    num_envs, horizon, mini_epochs, n_updates = [int(x) for x in g["meta"]]
    meta = dict(num_envs=num_envs, horizon=horizon, mini_epochs=mini_epochs, n_updates=n_updates,
                units=[int(x) for x in g["units"]], priv_units=[int(x) for x in g["priv_units"]])
    init = OrderedDict((k[len("init/"):], torch.from_numpy(v)) for k, v in g.items() if k.startswith("init/"))
    return g, meta, init


def load_ckpt():
    """teacher_shared_ckpt.npz as the nested dict the reference's PPO.save wrote (+ units, priv_units)."""
    z = np.load(os.path.join(GOLDEN, "teacher_shared_ckpt.npz"))
    ck = {}
    for k in z.files:
        if "/" in k:
            top, name = k.split("/", 1)
            ck.setdefault(top, OrderedDict())[name] = torch.from_numpy(z[k])
    return ck, [int(x) for x in z["units"]], [int(x) for x in z["priv_units"]]
