"""Shared by the loss-stage branch tests (test_loss_branches_cpu.py, test_gpu_loss_branches.py): an OFF-POLICY teacher
problem, the cases, a float64 restatement of one minibatch's loss and gradient, and the two conditions a case must meet
before a comparison on it means anything (census, near_kink).  Nothing here needs a GPU; each case's oracle walk is
computed once per process and shared.

Why: every other update test starts from oracle.synth.teacher_problem, where the old policy IS the current one (ratios
exactly 1, v - v_old near 0), sigma is the zero vector (sig = var = 1, logsc = 0, the same for every action dimension),
mu.bias is zero and mu.weight has gain 0.01 (|mu| << 1.1: the lower bounds term never switches on), and the
hyper-parameters are the defaults (entropy_coef 0).  The formulas of csrc/ppo_loss.h section 1 that differ from their
wrong neighbours only off that point -- x / var against x / sig, logstd[q] against logstd[0], the sign of blo, the
clipped branches of both losses for both signs, the entropy term of d_sigma -- are compared here.

Conditions (asserted by both test modules, for every minibatch compared):
  * each of the eight clip classes of `census` holds at least CLASS_FLOOR of the minibatch, and mu > 1.1 holds at least
    MU_FLOOR of the (sample, action) entries;
  * near_kink == 0: no sample within TAU of a discontinuity of the gradient, so the fp32 kernels and the float64
    reference take the same branch for every sample (their ratios / values differ by ~1e-6) and no sample is excused.
The seeds in CASES were chosen so that both hold; a changed seed fails the condition, not the comparison."""
import functools
from collections import OrderedDict
from types import SimpleNamespace

import torch

PRIV, OBS = 64, 15
PRIV_UNITS = [24, 16, 8]
HP = dict(e_clip=0.15, critic_coef=2.0, entropy_coef=0.01, bounds_loss_coef=0.05)
HP_ZERO = dict(HP, entropy_coef=0.0, bounds_loss_coef=0.0)
TAU = 1e-4
CLASS_FLOOR, MU_FLOOR = 0.03, 0.05
SOFT_BOUND = 1.1

CLASSES = ("ratio<lo adv<0", "ratio<lo adv>0", "ratio>hi adv>0", "ratio>hi adv<0",
           "dv>e l1>l2", "dv>e l1<l2", "dv<-e l1>l2", "dv<-e l1<l2")

# kernel: the profiler class that must run ("k_loss" counts k_loss_packed<MAXJ> (act <= 7) and k_loss<MAXJ> (act == 8);
# MAXJ = 1 | 2 | 4 follows from ceil(units[-1] / 64) in loss_stage), and the instantiation the shape selects there
CASES = {
    # name: (N, T, E), act, units, profiler class, instantiation, seed, force the sign of alternate mu.bias entries, hp
    "fused_150": ((100, 3, 2), 3, [64, 32, 128], "k_trunk_loss", "k_trunk_loss", 15, False, HP),   # two tiles + a ragged one
    "fused_50_act7": ((50, 5, 5), 7, [40, 96, 128], "k_trunk_loss", "k_trunk_loss", 13, False, HP),  # one partial tile
    "fused_257": ((257, 2, 2), 6, [32, 128], "k_trunk_loss", "k_trunk_loss", 16, False, HP),       # 4 tiles + one row
    "packed2_act7": ((96, 4, 3), 7, [48, 40, 100], "k_loss", "k_loss_packed<2>", 11, False, HP),
    "packed1_act3": ((96, 4, 3), 3, [48, 40, 24], "k_loss", "k_loss_packed<1>", 12, False, HP),
    "packed4_act6": ((96, 4, 3), 6, [48, 40, 200], "k_loss", "k_loss_packed<4>", 14, False, HP),
    "rows1_act8": ((96, 4, 3), 8, [48, 40, 24], "k_loss", "k_loss<1>", 13, False, HP),
    "rows2_act8": ((96, 4, 3), 8, [48, 40, 128], "k_loss", "k_loss<2>", 11, False, HP),            # the fused kernel's width
    "rows4_act8": ((96, 4, 3), 8, [48, 40, 200], "k_loss", "k_loss<4>", 16, False, HP),
    # the first shape with both optional terms switched off (oracle/teacher.py's zero-coefficient branch)
    "fused_150_zero_coef": ((100, 3, 2), 3, [64, 32, 128], "k_trunk_loss", "k_trunk_loss", 15, False, HP_ZERO),
}


def expected_instantiation(act, units):
    """What loss_stage / make_plan (csrc/ppo_loss.h section 5, csrc/teacher.h) launch for a shape, restated."""
    H = units[-1]
    if len(units) >= 2 and H == 128 and act <= 7 and units[-2] % 32 == 0:
        return "k_trunk_loss"
    maxj = 1 if H <= 64 else (2 if H <= 128 else 4)
    return f"k_loss_packed<{maxj}>" if act <= 7 else f"k_loss<{maxj}>"


def off_policy_problem(N, T, units, priv_units, act_dim, seed, obs_dim=OBS, force_bias_sign=False):
    """(init, ro, perm): synth.teacher_problem(done_p=0.1) moved off the freshly initialised policy.

    Parameters: sigma = linspace(-0.7, 0.4, act) in a random order (every action dimension its own sigma, none 1);
    mu.weight x 100 (gain 1: |mu| reaches the soft bound 1.1); mu.bias = 0.8 randn (force_bias_sign: alternate entries
    made +, -, +, ... so that at least one dimension sits on the positive side); every *_mlp bias 0.05 randn;
    value.bias stays 0.  Rollout, recomputed with THAT network on inputs normalised by fresh running statistics: the
    old policy is a perturbed copy of the current one (old mu = mu + 0.12 sigma randn, old sigma = sigma exp(0.15
    randn) per action dimension), actions are drawn from the old policy, neglogpacs are the old policy's, old values
    are the network's plus 0.5 randn."""
    from oracle import synth, teacher as ot
    init, ro, perm = synth.teacher_problem(N, T, units, priv_units, obs_dim=obs_dim, act_dim=act_dim, seed=seed, done_p=0.1)
    g = torch.Generator().manual_seed(seed + 77)
    init = OrderedDict((k, v.clone().float()) for k, v in init.items())
    init["sigma"] = torch.linspace(-0.7, 0.4, act_dim)[torch.randperm(act_dim, generator=g)].contiguous()
    init["mu.weight"] = init["mu.weight"] * 100.0
    bias = 0.8 * torch.randn(act_dim, generator=g)
    if force_bias_sign:
        bias = bias.abs() * torch.tensor([1.0 if q % 2 == 0 else -1.0 for q in range(act_dim)])
    init["mu.bias"] = bias
    for k in init:
        if "_mlp." in k and k.endswith("bias"):
            init[k] = 0.05 * torch.randn(init[k].shape, generator=g)
    ro = dict(ro)
    rs_o, rs_p, rs_v = ot.RmsState(obs_dim), ot.RmsState(PRIV), ot.RmsState(1)
    with torch.no_grad():
        mu, logstd, value, _ = ot.actor_critic(init, rs_o.normalize(ro["obses"].reshape(-1, obs_dim)),
                                               rs_p.normalize(ro["priv_info"].reshape(-1, PRIV)), len(priv_units), len(units))
        sigma = torch.exp(logstd)
        mus_old = mu + 0.12 * sigma * torch.randn(mu.shape, generator=g)
        sigmas_old = sigma * torch.exp(0.15 * torch.randn(act_dim, generator=g))
        actions = mus_old + sigmas_old * torch.randn(mu.shape, generator=g)
        nlp = ot.gaussian_neglogp(actions, mus_old, sigmas_old, torch.log(sigmas_old))
        values = rs_v.unnormalize(value) + 0.5 * torch.randn(value.shape, generator=g)
    ro["mus"], ro["sigmas"] = mus_old.reshape(T, N, act_dim).contiguous(), sigmas_old.reshape(T, N, act_dim).contiguous()
    ro["actions"] = actions.reshape(T, N, act_dim).contiguous()
    ro["neglogpacs"] = nlp.reshape(T, N).contiguous()
    ro["values"] = values.reshape(T, N, 1).contiguous()
    return init, ro, perm


def reference64(orc, i):
    """Minibatch i of the oracle's NEXT step in float64: loss (frozen_ppo.py:543-563) and its gradient by autograd on
    .double() copies of the oracle's parameters, inputs normalised by clones of its running statistics advanced over
    this minibatch (what the step itself does, frozen_ppo.py:521-522).  The oracle is left untouched.

    Returns grad (flat, state_dict order; zeros where a tensor gets none), means (actor, critic, bounds, entropy,
    policy_kl), mu, sigma, and per sample what census / near_kink read: ratio, adv, dv = v - v_old, l1, l2."""
    from oracle import teacher as ot
    h, d = orc.hp, orc.data
    idx = orc.perm[i * orc.mb:(i + 1) * orc.mb]
    rms_o, rms_p = orc.rms_obs.clone(), orc.rms_priv.clone()
    obs, priv = rms_o(d["obses"][idx], True).double(), rms_p(d["priv_info"][idx], True).double()
    p = OrderedDict((k, v.detach().double().requires_grad_(True)) for k, v in orc.p.items())
    nlp, values, entropy, mu, sigma = ot.forward_train(p, obs, priv, d["actions"][idx].double(), len(orc.priv_units),
                                                       len(orc.units))
    adv, old_nlp = d["advantages"][idx].double(), d["neglogpacs"][idx].double()
    v_old, R = d["values"][idx].double(), d["returns"][idx].double()
    e = h["e_clip"]
    lo, hi = 1.0 - e, 1.0 + e
    ratio = torch.exp(old_nlp - nlp)
    a_loss = torch.max(-adv * ratio, -adv * ratio.clamp(lo, hi))
    dv = values - v_old
    l1, l2 = (values - R) ** 2, (v_old + dv.clamp(-e, e) - R) ** 2
    c_loss = torch.max(l1, l2)
    if h["bounds_loss_coef"] > 0:
        b_loss = (torch.clamp_max(mu - SOFT_BOUND, 0.0) ** 2 + torch.clamp_max(-mu + SOFT_BOUND, 0.0) ** 2).sum(-1)
    else:
        b_loss = torch.zeros_like(a_loss)
    a_m, c_m, b_m, e_m = a_loss.mean(), c_loss.mean(), b_loss.mean(), entropy.mean()
    loss = a_m + 0.5 * c_m * h["critic_coef"] - e_m * h["entropy_coef"] + b_m * h["bounds_loss_coef"]
    gs = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    grad = torch.cat([(g_ if g_ is not None else torch.zeros_like(q)).reshape(-1) for g_, q in zip(gs, p.values())])
    with torch.no_grad():
        kl = ot.policy_kl(mu, sigma, d["mus"][idx].double(), d["sigmas"][idx].double())
    return SimpleNamespace(grad=grad.detach(), means=[x.item() for x in (a_m, c_m, b_m, e_m, kl)], mu=mu.detach(),
                           sigma=sigma.detach(), ratio=ratio.detach(), adv=adv, dv=dv.detach().squeeze(1),
                           l1=l1.detach().squeeze(1), l2=l2.detach().squeeze(1), e_clip=e, rows=idx.clone())


def census(ref):
    """({class: share of the minibatch} in the order of CLASSES, share of (sample, action) entries with mu > 1.1)."""
    e = ref.e_clip
    lo, hi = 1.0 - e, 1.0 + e
    r, a, dv, l1, l2 = ref.ratio, ref.adv, ref.dv, ref.l1, ref.l2
    masks = [(r < lo) & (a < 0), (r < lo) & (a > 0), (r > hi) & (a > 0), (r > hi) & (a < 0),
             (dv > e) & (l1 > l2), (dv > e) & (l1 < l2), (dv < -e) & (l1 > l2), (dv < -e) & (l1 < l2)]
    return OrderedDict((nm, m.double().mean().item()) for nm, m in zip(CLASSES, masks)), \
        (ref.mu > SOFT_BOUND).double().mean().item()


def near_kink(ref, tau=TAU):
    """Samples within tau of a discontinuity of the gradient: the ratio on 1 -+ e_clip, |v - v_old| on e_clip, or the
    two value-loss branches tied outside the clip range.  (The bounds term is C1: no margin needed.)"""
    e = ref.e_clip
    r, dv = ref.ratio, ref.dv
    amb_p = ((r - (1.0 - e)).abs() < tau) | ((r - (1.0 + e)).abs() < tau)
    amb_v = ((dv.abs() - e).abs() < tau) | ((dv.abs() > e) & ((ref.l1 - ref.l2).abs() < tau))
    return int((amb_p | amb_v).sum().item())


@functools.lru_cache(maxsize=None)
def walk(name):
    """The oracle walked through the first mini-epoch of a case, one optimizer step per minibatch.  Per step: the
    parameters and Adam moments the step starts from (what the GPU test loads into its engine), the float64 reference
    of its minibatch, then the fp32 oracle's own step (update(record_grads=1, max_steps=1, start_step=slot)): its
    recorded gradient, statistics and the parameters after it.  Computed once; treat the result as read-only."""
    from oracle import teacher as ot
    (N, T, E), act, units, _, _, seed, force, hp = CASES[name]
    init, ro, perm = off_policy_problem(N, T, units, PRIV_UNITS, act, seed, force_bias_sign=force)
    orc = ot.TeacherOracle(init, perm, N, T, E, units, PRIV_UNITS, obs_dim=OBS, act_dim=act, **hp)
    orc.prepare(ro)
    steps = []
    for slot in range(orc.n_mb):
        s = SimpleNamespace()
        s.params = OrderedDict((k, v.detach().clone()) for k, v in orc.p.items())
        s.adam = OrderedDict((k, (m.clone(), v.clone())) for k, (m, v) in orc.adam_state().items())
        s.param_norm = torch.cat([v.double().reshape(-1) for v in s.params.values()]).norm().item()
        s.ref = reference64(orc, slot)
        st = orc.update(record_grads=1, max_steps=1, start_step=slot)
        s.grad32 = st["grads"][0]
        s.b_loss32 = st["b_losses"][0].item()
        s.params_after = orc.flat_params().clone()
        steps.append(s)
    return SimpleNamespace(init=init, ro=ro, perm=perm, steps=steps, hp=dict(hp), lr=orc.hp["lr"],
                           mus=orc.data["mus"].detach().clone(), sigmas=orc.data["sigmas"].detach().clone())
