"""Rollouts for the data-dependent front of the teacher update (GAE, advantage / value normalisation, the minibatch
gather and the running normalisers) OFF the unit-normal data of oracle.synth.teacher_problem.  Shared by
test_teacher_prep_cpu.py and test_gpu_teacher_prep.py; nothing here needs a GPU.

The rollout is synth.teacher_problem's (values, mus, sigmas and neglogpacs stay those of the initial network), with
``obses`` and ``priv_info`` overwritten column by column from a seeded CPU generator.  Column kinds (z is N(0, 1)):

  unit    z                              the only kind every other teacher test sees
  offset  1000 + 0.01 z                  mean >> std: cancellation in sum(x^2) - n m^2
  far     1e5 + 0.05 z                   the same, at fp32's resolution of the data (ulp(1e5) = 0.0078)
  wide    1e4 z
  tiny    1e-6 z                         var << eps: the denominator is sqrt(eps)
  const   0.37 exactly                   var exactly 0
  zero    0 exactly
  tail    z, 2 % of the entries +-50     entries the +-5 clamp acts on, both signs
  flag    0 / 1 with p = 0.02            sparse; a set flag normalises to ~7 and clamps
  clock   t + 0.01 z                     correlated with the time index: minibatch moments differ from the global ones

Columns are drawn in float64 and rounded to fp32 once; what the tests compare against is computed from those fp32
values in float64 (tests/teacher_prep_ref.py)."""
import functools

import torch

KINDS = ("unit", "offset", "far", "wide", "tiny", "const", "zero", "tail", "flag", "clock")
UNITS, PRIV_UNITS, ACT = [64, 32], [32, 8], 6

# name: (N, T, mini_epochs), obs_dim, priv_dim, (gamma, tau), rms_eps, reward/value variant
CASES = {
    # mb = 300: 10 gather blocks of 32 rows, the last with 12 -> the strided partial sum (b = j; b += 8) takes a second lap
    "mb300": ((75, 4, 1), 15, 64, (0.9, 0.8), 1e-5, False),
    # N = 300: two k_gae blocks, the second with 44 envs; n_mb = 3; rewards 1 + 0.1 z and values + 100
    "gae2": ((300, 3, 3), 15, 64, (0.998, 0.95), 1e-5, True),
    # mb = 37: one full gather block and 5 rows; 25 optimizer steps; an epsilon off the default
    "rows37": ((37, 5, 5), 15, 64, (1.0, 1.0), 1e-3, False),
    # D = 170 > 128: the second c0 pass of k_mb_moments and the second lap of k_rms_traj's 128 threads; mb = 150, n_mb = 2
    "wide170": ((75, 4, 2), 20, 150, (0.95, 0.0), 1e-5, False),
}
GAE_PAIRS = ((0.9, 0.8), (0.998, 0.95), (1.0, 1.0), (0.95, 0.0))


def kinds_for(dim, first):
    """Column kinds of a ``dim``-wide input: KINDS in order starting at ``first``, repeated (dim >= 10: all appear)."""
    assert dim >= len(KINDS)
    return [KINDS[(first + c) % len(KINDS)] for c in range(dim)]


def column(kind, T, N, g):
    """One (T, N) column in float64."""
    z = torch.randn(T, N, generator=g, dtype=torch.float64)
    if kind == "unit":
        return z
    if kind == "offset":
        return 1000.0 + 0.01 * z
    if kind == "far":
        return 1e5 + 0.05 * z
    if kind == "wide":
        return 1e4 * z
    if kind == "tiny":
        return 1e-6 * z
    if kind == "const":
        return torch.full_like(z, 0.37)
    if kind == "zero":
        return torch.zeros_like(z)
    if kind == "tail":
        n_out = max(2, 2 * int(round(0.01 * T * N)))          # 2 % of the entries, half of them each sign
        where = torch.randperm(T * N, generator=g)[:n_out]
        flat = z.reshape(-1)
        flat[where[0::2]] = 50.0
        flat[where[1::2]] = -50.0
        return flat.reshape(T, N)
    if kind == "flag":
        return (torch.rand(T, N, generator=g, dtype=torch.float64) < 0.02).double()
    if kind == "clock":
        return torch.arange(T, dtype=torch.float64)[:, None] + 0.01 * z
    raise KeyError(kind)


def columns(kinds, T, N, g):
    """(T, N, len(kinds)) fp32."""
    return torch.stack([column(k, T, N, g) for k in kinds], dim=-1).float().contiguous()


def obs_kinds(obs_dim):
    return kinds_for(obs_dim, 0)


def priv_kinds(priv_dim):
    return kinds_for(priv_dim, 3)


def rollout(N, T, obs_dim=15, priv_dim=64, seed=1234, value_variant=False, done_p=0.05):
    """(init params, rollout, perm): synth.teacher_problem with the inputs replaced by the column kinds.
    value_variant: rewards 1 + 0.1 z and every value (last_values too) shifted by +100."""
    from oracle import synth
    init, ro, perm = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, obs_dim=obs_dim, priv_dim=priv_dim, act_dim=ACT,
                                           seed=seed, done_p=done_p)
    g = torch.Generator().manual_seed(seed + 7919)
    ro = dict(ro)
    ro["obses"] = columns(obs_kinds(obs_dim), T, N, g)
    ro["priv_info"] = columns(priv_kinds(priv_dim), T, N, g)
    if value_variant:
        ro["rewards"] = (1.0 + 0.1 * torch.randn(T, N, 1, generator=g, dtype=torch.float64)).float().contiguous()
        ro["values"] = (ro["values"] + 100.0).contiguous()
        ro["last_values"] = (ro["last_values"] + 100.0).contiguous()
    return init, ro, perm


def shifted(ro):
    """The rollout of a SECOND update: every input column scaled by 2 and moved by 3 of its own (float64) std."""
    out = dict(ro)
    for k in ("obses", "priv_info"):
        x = ro[k].double()
        std = x.reshape(-1, x.shape[-1]).std(0)
        out[k] = (2.0 * x + 3.0 * std).float().contiguous()
    return out


def held_out_rows(rows, obs_dim, priv_dim, seed):
    """(rows, obs_dim), (rows, priv_dim): fresh draws of the same column kinds (tail outliers included) for inference."""
    g = torch.Generator().manual_seed(seed)
    return columns(obs_kinds(obs_dim), rows, 1, g)[:, 0], columns(priv_kinds(priv_dim), rows, 1, g)[:, 0]


def warm_state(kinds, T, N, seed, count=1e8):
    """A normaliser that has seen 1e8 samples: float64 (mean, var, count) with the moments of a DIFFERENT draw of the
    same column kinds."""
    g = torch.Generator().manual_seed(seed)
    x = columns(kinds, T, N, g).double().reshape(T * N, len(kinds))
    return x.mean(0), x.var(0), torch.tensor(count, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def case(name, seed=1234):
    """The named case: dict(N, T, E, obs_dim, priv_dim, gamma, tau, rms_eps, init, ro, perm)."""
    (N, T, E), obs_dim, priv_dim, (gamma, tau), eps, vv = CASES[name]
    init, ro, perm = rollout(N, T, obs_dim, priv_dim, seed=seed, value_variant=vv)
    return dict(N=N, T=T, E=E, obs_dim=obs_dim, priv_dim=priv_dim, gamma=gamma, tau=tau, rms_eps=eps, init=init, ro=ro,
                perm=perm, mb=N * T // E, n_mb=(N * T) // (N * T // E))
