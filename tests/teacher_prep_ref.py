"""Float64 restatement of the data-dependent front of the teacher update: experience.py:242-263 (GAE, advantages),
frozen_ppo.py:717-725 (the two value-normaliser updates), frozen_ppo.py:521-522 (the per-step input normalisers) and
running_mean_std.py:48-93 (Chan merge, normalise + clamp, un-normalise).  Nothing is rounded to fp32 inside: the fp32
rollout is widened once, gamma * tau, the batch moments (two-pass) and the running state are doubles throughout.  This is
the TRUTH the GPU tests compare with; the fp32 CPU oracle (oracle/teacher.py) is run next to it only to measure how far the
reference's own arithmetic is from it (``oracle_*`` below), which is what the GPU bounds are built from.

Also here: the bound terms (State64.e_mean / e_var / floor_norm, floor_norm: what the fp32 operations the reference itself
performs cost; ``bound``: the larger of that and 3 x the oracle's error) and
the float64 loss + gradient of one minibatch fed the restatement's rows."""
from collections import OrderedDict
from types import SimpleNamespace

import torch

U = 2.0 ** -24      # fp32 unit roundoff


# ---- running_mean_std.py:48-93 -------------------------------------------------------------------------------------
class State64:
    """mean / var / count in float64, and next to them e_mean / e_var: how far the REFERENCE's state may be from this
    one because its batch moments are fp32 tensors (x.mean(0), x.var(0)) -- the floor of the bounds, carried through the
    merges to first order:
        b_mean rounds by 2^-24 |b_mean|, b_var by 2^-23 b_var (its own rounding and that of the mean inside it);
        e_mean' = (e_mean count + 2^-24 |b_mean| n) / tot
        e_var'  = (e_var count + 2^-23 b_var n + (2 |delta| e_delta + e_delta^2) count n / tot) / tot,
        e_delta = 2^-24 |b_mean| + e_mean.
    After ONE merge into the fresh state (mean 0, count 1) these are 2^-24 |mean| and 2^-23 var + (2^-24 mean)^2 to
    first order; over several merges they also cover batch means that cancel in the running mean (tail columns: batch
    means of +-2.6 leave a running mean of 0.03), where no fp32 batch mean, however well rounded, is within 2^-24 of the
    running mean."""

    def __init__(self, mean, var, count, e_mean=None, e_var=None):
        self.mean, self.var, self.count = mean.double().clone(), var.double().clone(), count.double().clone()
        self.e_mean = torch.zeros_like(self.mean) if e_mean is None else e_mean.clone()
        self.e_var = torch.zeros_like(self.var) if e_var is None else e_var.clone()

    @classmethod
    def fresh(cls, dim):
        return cls(torch.zeros(dim), torch.ones(dim), torch.ones(()))

    def clone(self):
        return State64(self.mean, self.var, self.count, self.e_mean, self.e_var)

    def packed(self):
        return torch.cat([self.mean, self.var, self.count.reshape(1)])

    def merge(self, x):
        """running_mean_std.py:48-65 with exact two-pass batch moments (unbiased var)."""
        x = x.double()
        n = x.shape[0]
        b_mean = x.mean(0)
        b_var = ((x - b_mean) ** 2).sum(0) / (n - 1)
        delta = b_mean - self.mean
        tot = self.count + n
        m2 = self.var * self.count + b_var * n + delta ** 2 * self.count * n / tot
        e_delta = U * b_mean.abs() + self.e_mean
        self.e_var = (self.e_var * self.count + 2.0 * U * b_var * n
                      + (2.0 * delta.abs() * e_delta + e_delta ** 2) * self.count * n / tot) / tot
        self.e_mean = (self.e_mean * self.count + U * b_mean.abs() * n) / tot
        self.mean, self.var, self.count = self.mean + delta * n / tot, m2 / tot, tot

    def den(self, eps):
        return torch.sqrt(self.var + eps)

    def normalize(self, x, eps, clamp=True):
        y = (x.double() - self.mean) / self.den(eps)
        return torch.clamp(y, -5.0, 5.0) if clamp else y

    def unnormalize(self, y, eps):
        return self.den(eps) * torch.clamp(y.double(), -5.0, 5.0) + self.mean

    def floor_norm(self, x, eps, y):
        """A normalised entry y = (x - m) / d as the reference forms it in fp32 from ITS state: m is off by e_mean and
        rounds, x - m rounds (2^-24 (|x| + |m|) + e_mean, over d), d is off by e_var / 2d, and d, the division and the
        result round (3 * 2^-24 |y|)."""
        d = self.den(eps)
        return (U * (x.double().abs() + self.mean.abs()) + self.e_mean) / d + (3.0 * U + self.e_var / (2.0 * d * d)) * y.abs()


def env_major(x):
    s = x.shape
    return x.transpose(0, 1).reshape(s[0] * s[1], *s[2:])


# ---- experience.py:242-263 + frozen_ppo.py:717-725 ----------------------------------------------------------------------
def gae64(rewards, values, dones, last_values, gamma, tau):
    r, v, lv = rewards.double(), values.double(), last_values.double()
    nd = 1.0 - dones.double()
    T = r.shape[0]
    out = torch.zeros_like(r)
    lam = torch.zeros_like(lv)
    for t in reversed(range(T)):
        nxt = lv if t == T - 1 else v[t + 1]
        nn_ = nd[t].unsqueeze(1)
        delta = r[t] + gamma * nxt * nn_ - v[t]
        lam = delta + gamma * tau * nn_ * lam
        out[t] = lam + v[t]
    return out


def prepare64(ro, rms_value, gamma, tau, eps, normalize_value=True):
    """-> returns_raw (T, N, 1), then env-major: adv_raw, adv_mean, adv_den, advantages (B,), values_n, returns_n (B, 1),
    and the value normaliser's state after each of its two merges (val_states)."""
    ret = gae64(ro["rewards"], ro["values"], ro["dones"], ro["last_values"], gamma, tau)
    v, r = env_major(ro["values"].double()), env_major(ret)
    adv = (r - v).squeeze(1)
    am, ad = adv.mean(), adv.std() + 1e-8                       # unbiased std (experience.py:261-262)
    st = rms_value.clone()
    states = []
    if normalize_value:
        st.merge(v)
        states.append(st.clone())
        v_n = st.normalize(v, eps)
        st.merge(r)
        states.append(st.clone())
        r_n = st.normalize(r, eps)
    else:
        v_n, r_n = v, r
    return SimpleNamespace(returns_raw=ret, adv_raw=adv, adv_mean=am, adv_den=ad, advantages=(adv - am) / ad, values=v,
                           returns=r, values_n=v_n, returns_n=r_n, val_states=states, rms_value=st)


# ---- frozen_ppo.py:521-522 over the E * n_mb optimizer steps ---------------------------------------------------------------
def trajectory64(ro, perm, E, mb, rms_obs, rms_priv, eps, clamp=True, steps=None):
    """Per optimizer step k (minibatch k % n_mb in the order ``perm`` defines): Chan merge of the minibatch's exact moments,
    then the minibatch normalised with the merged state.  -> list of SimpleNamespace(idx, obs_state, priv_state, obs, priv,
    raw_obs, raw_priv); the states passed in are left untouched."""
    o, p = env_major(ro["obses"]).double(), env_major(ro["priv_info"]).double()
    so, sp = rms_obs.clone(), rms_priv.clone()
    n_mb = o.shape[0] // mb
    out = []
    for k in range(E * n_mb if steps is None else steps):
        i = k % n_mb
        idx = perm[i * mb:(i + 1) * mb].long()
        xo, xp = o[idx], p[idx]
        so.merge(xo)
        sp.merge(xp)
        out.append(SimpleNamespace(idx=idx, obs_state=so.clone(), priv_state=sp.clone(), raw_obs=xo, raw_priv=xp,
                                   obs=so.normalize(xo, eps, clamp), priv=sp.normalize(xp, eps, clamp)))
    return out


# ---- the fp32 CPU oracle on the same input (ONLY to size the bounds) --------------------------------------------------------
def oracle_state(rms):
    return State64(rms.mean, rms.var, rms.count)


def oracle_rms(state64, eps):
    from oracle.teacher import RmsState
    r = RmsState(state64.mean.shape[0], eps)
    r.mean, r.var, r.count = state64.mean.clone(), state64.var.clone(), state64.count.clone()
    return r


def oracle_trajectory(ro, perm, E, mb, rms_obs, rms_priv, eps, steps=None):
    """trajectory64's steps through oracle.teacher.RmsState (fp32 batch moments and rows, fp64 state)."""
    o, p = env_major(ro["obses"]), env_major(ro["priv_info"])
    so, sp = oracle_rms(rms_obs, eps), oracle_rms(rms_priv, eps)
    n_mb = o.shape[0] // mb
    out = []
    for k in range(E * n_mb if steps is None else steps):
        i = k % n_mb
        idx = perm[i * mb:(i + 1) * mb].long()
        yo, yp = so(o[idx], train=True), sp(p[idx], train=True)
        out.append(SimpleNamespace(obs_state=oracle_state(so), priv_state=oracle_state(sp), obs=yo, priv=yp))
    return out


def oracle_prepare(ro, rms_value, gamma, tau, eps):
    """oracle.teacher's prepare arithmetic (fp32) from a given value-normaliser state."""
    from oracle import teacher as ot
    ret = ot.gae_returns(ro["rewards"], ro["values"], ro["dones"], ro["last_values"], gamma, tau)
    v, r = ot.env_major(ro["values"]), ot.env_major(ret)
    adv = ot.normalized_advantages(r, v)
    st = oracle_rms(rms_value, eps)
    v_n = st(v, train=True)
    r_n = st(r, train=True)
    return SimpleNamespace(returns_raw=ret, advantages=adv, values_n=v_n, returns_n=r_n, rms_value=oracle_state(st))


# ---- bound terms ----------------------------------------------------------------------------------------------------
def floor_norm(x, mean, den, y):
    """An advantage y = (x - m) / d, m and d formed in fp32 from the tensor itself: m and x - m each round
    (2^-24 (|x| + |m|) / d), then d, the division and the result (3 * 2^-24 |y|)."""
    return U * (x.abs() + mean.abs()) / den + 3.0 * U * y.abs()


def bound(floor, oracle_err, cols=False):
    """max(floor, 3 x the fp32 oracle's own error): per column (dim 0 reduced) when ``cols``, else over the tensor."""
    oe = oracle_err.double().abs()
    assert torch.isfinite(oe).all(), "the fp32 oracle's own error is not finite"
    if not cols:
        oe = oe.max()
    elif oe.dim() == 2:
        oe = oe.amax(0, keepdim=True)          # rows of a minibatch: the column's worst entry
    return torch.maximum(floor.double(), 3.0 * oe)


def worst_ratio(got, truth, bnd):
    """max over all entries of |got - truth| / bound, with 0 / 0 = 0 (an exact entry under a zero bound passes)."""
    err = (got.double() - truth).abs()
    assert torch.isfinite(err).all(), "non-finite entries"
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return float(r.max())


# ---- one minibatch's loss and gradient in float64 (frozen_ppo.py:543-564) ----------------------------------------------------
def step_loss64(params, obs_n, priv_n, idx, ro, prep, hp, n_priv_layers, n_layers):
    """Loss means (actor, critic, bounds, entropy) and the flat gradient (state_dict order) of the minibatch ``idx`` on
    float64 copies of ``params``, fed the normalised rows given."""
    from oracle import teacher as ot
    p = OrderedDict((k, v.detach().double().requires_grad_(True)) for k, v in params.items())
    actions = env_major(ro["actions"]).double()[idx]
    old_nlp = env_major(ro["neglogpacs"]).double()[idx]
    nlp, values, entropy, mu, sigma = ot.forward_train(p, obs_n, priv_n, actions, n_priv_layers, n_layers)
    adv, v_old, R = prep.advantages[idx], prep.values_n[idx], prep.returns_n[idx]
    e = hp["e_clip"]
    ratio = torch.exp(old_nlp - nlp)
    a_loss = torch.max(-adv * ratio, -adv * ratio.clamp(1.0 - e, 1.0 + e))
    c_loss = torch.max((values - R) ** 2, (v_old + (values - v_old).clamp(-e, e) - R) ** 2)
    if hp["bounds_loss_coef"] > 0:
        b_loss = (torch.clamp_max(mu - 1.1, 0.0) ** 2 + torch.clamp_max(-mu + 1.1, 0.0) ** 2).sum(-1)
    else:
        b_loss = torch.zeros_like(a_loss)
    means = [x.mean() for x in (a_loss, c_loss, b_loss, entropy)]
    loss = means[0] + 0.5 * means[1] * hp["critic_coef"] - means[3] * hp["entropy_coef"] + means[2] * hp["bounds_loss_coef"]
    gs = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    grad = torch.cat([(g if g is not None else torch.zeros_like(q)).reshape(-1) for g, q in zip(gs, p.values())])
    return SimpleNamespace(means=[float(m.detach()) for m in means], grad=grad.detach())


def clamp_sensitivity(with_clamp, without):
    """How far step_loss64 moves when the rows are not clamped, in units of the bounds the GPU test holds the step-0
    record to: (max over gradient entries of |move| / (2e-4 max|g| + 2e-3 |g|), |critic-loss move| / (2e-4 |c_loss|))."""
    g, g2 = with_clamp.grad, without.grad
    bnd = 2e-4 * g.abs().max() + 2e-3 * g.abs()
    return float(((g2 - g).abs() / bnd).max()), abs(without.means[1] - with_clamp.means[1]) / (2e-4 * abs(with_clamp.means[1]))


def infer64(params, obs_n, priv_n, n_priv_layers, n_layers):
    """(mu, normalised value, latent) of oracle.teacher.actor_critic in float64 on rows already normalised."""
    from oracle import teacher as ot
    p = {k: v.detach().double() for k, v in params.items()}
    with torch.no_grad():
        mu, _, value, lat = ot.actor_critic(p, obs_n.double(), priv_n.double(), n_priv_layers, n_layers)
    return mu, value, lat
