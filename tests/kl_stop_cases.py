"""Shared by the KL early-stopping tests (test_kl_stop_cpu.py, test_gpu_kl_stop.py): the cases and the CPU driver -- the
reference's loop with the breaks of frozen_ppo.py:578-581 and :642-643 live, built from the oracle's public pieces only.

Before oracle step s the driver peeks: it clones the two RmsStates, normalises the step's minibatch with the clones
(which ingest it, as :521-522 do), runs oracle.teacher.forward_train under no_grad and forms the estimator of :568-569,
mean((exp(d) - 1) - d) with d = neglogp_new - neglogp_old, in fp32 (what the reference computes) and in float64 (what
the device's per-step figure is held to).  If the fp32 figure is strictly above 1.5 * kl_threshold the step stops the
update: the minibatch is ingested into the real normalisers and nothing else is called.  Otherwise
orc.update(start_step=s, max_steps=1) runs the step.  The driver checks itself: the policy_kl it peeked must
torch.equal the oracle's step_kls entry.

Condition on every case (assert_margins, asserted where a case is used, before any GPU comparison): every step before
the stop lies at least 10 % below 1.5 * thr, the stop step at least 10 % above it -- five orders of magnitude more than
the estimator tolerance the GPU is held to, so the device takes the oracle's decision or the estimator test fails first.
The combined case also keeps lr_schedule_cases.MARGIN on every rate decision.

Each case's oracle run is computed once per process and shared, read-only; nothing here needs a GPU."""
import functools

import numpy as np
import torch

from tests import lr_schedule_cases as L

MARGIN = 0.10
ACT8 = 8

CASES = {
    # name: lr_schedule_cases-style shape entry + lr0, kl_threshold, adaptive learning rate, action dimensions
    # A: 256 x 16, E 4, default widths (k_trunk_loss), mb 1024, 16 steps.  Estimator 2.92e-4 at step 5, 3.95e-4 at step 6
    "A": dict(shape=(256, 16, 4), units=L.DEFAULT_UNITS, priv_units=L.DEFAULT_PRIV_UNITS, lr=2.5e-4, thr=3.4e-4 / 1.5,
              contacts=(0, 0), stop=6),                                          # mid mini-epoch 1
    # B: the same shape at 3e-3: 3.53e-3 at step 1, 9.35e-3 at step 2
    "B": dict(shape=(256, 16, 4), units=L.DEFAULT_UNITS, priv_units=L.DEFAULT_PRIV_UNITS, lr=3e-3, thr=4e-3,
              contacts=(0, 0), stop=2),
    # C: 100 x 6, E 3, widths 48/40/24 (k_loss_packed, mb 200: ragged tile), 9 steps: 5.57e-3 at step 3, 1.01e-2 at step 4
    "C": dict(shape=(100, 6, 3), units=L.SMALL_UNITS, priv_units=L.SMALL_PRIV_UNITS, lr=5e-3, thr=5e-3,
              contacts=(0, 0), stop=4),
    # C's shape with ground-truth contacts: 1.20e-2 at step 5, 2.18e-2 at step 6 = the first step of mini-epoch 2
    "C_contacts": dict(shape=(100, 6, 3), units=L.SMALL_UNITS, priv_units=L.SMALL_PRIV_UNITS, lr=5e-3, thr=1.0667e-2,
                       contacts=(37, 8), stop=6),
    # eight actions off the default widths (k_loss: one lane per action): C's shape and rate.  2.90e-3 at step 2,
    # 9.09e-3 at step 3: 1.5 thr = 6e-3 sits between 2.90e-3 / 0.9 = 3.2e-3 and 9.09e-3 / 1.1 = 8.3e-3
    "act8": dict(shape=(100, 6, 3), units=L.SMALL_UNITS, priv_units=L.SMALL_PRIV_UNITS, lr=5e-3, thr=4e-3,
                 contacts=(0, 0), stop=3, act=ACT8),
    # A with a threshold nothing reaches: the update runs through
    "no_stop": dict(shape=(256, 16, 4), units=L.DEFAULT_UNITS, priv_units=L.DEFAULT_PRIV_UNITS, lr=2.5e-4, thr=1.0,
                    contacts=(0, 0), stop=None),
    # the stop together with lr_schedule: adaptive (the scheduler runs once more, on the partial mean, :630)
    # A's problem.  Mini-epoch 0: KL 8.94e-5 < 0.5 thr = 1.5e-4 (40 % off) -> the rate goes up to 3.75e-4; then 3.49e-4 at
    # step 5 and 5.35e-4 at step 6 around 1.5 thr = 4.5e-4 (0.9 x = 4.05e-4, 1.1 x = 4.95e-4); the scheduler's last call
    # sees the mean KL of steps 4 .. 6, 2.52e-4: 58 % off the nearer boundary, hold
    "adaptive": dict(shape=(256, 16, 4), units=L.DEFAULT_UNITS, priv_units=L.DEFAULT_PRIV_UNITS, lr=2.5e-4, thr=3e-4,
                     contacts=(0, 0), stop=6, adaptive=True),
}


def approx_kl(nlp, old_nlp):
    """frozen_ppo.py:568-569 as written, in fp32, and the float64 restatement of the same fp32 inputs."""
    d = nlp - old_nlp
    k32 = torch.mean((torch.exp(d) - 1) - d)
    d64 = nlp.double() - old_nlp.double()
    k64 = torch.mean((torch.exp(d64) - 1) - d64)
    return k32, k64


@functools.lru_cache(maxsize=None)
def case_problem(name):
    c = CASES[name]
    N, T, E = c["shape"]
    P, Ec = c["contacts"]
    if c.get("act", L.ACT) != L.ACT:
        from oracle import synth
        return synth.teacher_problem(N, T, c["units"], c["priv_units"], obs_dim=L.OBS, act_dim=c["act"], seed=L.SEED)
    return L.problem(N, T, c["units"], c["priv_units"], P, Ec)


def drive_oracle(name, thr=None, max_steps=None):
    """The oracle with the breaks live.  thr None: the case's own.  max_steps: stop driving after that many steps (for
    the step-count comparisons), without a break.
    Returns dict(stop: step or None, approx32 / approx64 / step_kls / entropies: per evaluated step (the stop step
    included), a_losses / c_losses / b_losses: per applied step, kls: the trainer's KL list, lrs / kl_seen: the rate
    after and the KL compared at each scheduler call (adaptive only), step_lr: the rate each applied step used, params,
    adam: flat final parameters and moments, rms_obs / rms_priv: (mean, var, count), mus / sigmas: the arena (B, act)
    env-major, idx_stop: the stop step's sample ids, thr)."""
    from oracle import teacher as ot
    c = CASES[name]
    thr = c["thr"] if thr is None else thr
    N, T, E = c["shape"]
    P, Ec = c["contacts"]
    act = c.get("act", L.ACT)
    adaptive = bool(c.get("adaptive", False))
    init, ro, perm = case_problem(name)
    orc = ot.TeacherOracle(init, perm, N, T, E, c["units"], c["priv_units"], obs_dim=L.OBS, act_dim=act, contact_points=P,
                           contact_emb=Ec, lr=c["lr"])
    orc.prepare(ro)
    d, n_mb, mb = orc.data, orc.n_mb, orc.mb
    n_pl, n_l = len(c["priv_units"]), len(c["units"])
    out = dict(stop=None, approx32=[], approx64=[], step_kls=[], entropies=[], a_losses=[], c_losses=[], b_losses=[],
               kls=[], lrs=[], kl_seen=[], step_lr=[], idx_stop=None, thr=thr)
    lr = c["lr"]
    total = E * n_mb if max_steps is None else max_steps
    ep_kls = []

    def end_of_mini_epoch():
        nonlocal lr
        kl = torch.stack(ep_kls).mean()
        out["kls"].append(kl.item())
        if adaptive:                                   # :630 sits between the inner break and the outer one
            lr = L.rule(lr, kl.item(), thr)
            out["lrs"].append(lr)
            out["kl_seen"].append(kl.item())

    for s in range(total):
        i = s % n_mb
        if i == 0:
            ep_kls = []
        orc.opt.param_groups[0]["lr"] = lr
        idx = orc.perm[i * mb:(i + 1) * mb]
        peek_o, peek_p = orc.rms_obs.clone(), orc.rms_priv.clone()
        with torch.no_grad():
            obs, priv = peek_o(d["obses"][idx], train=True), peek_p(d["priv_info"][idx], train=True)
            extra = (d["contacts"][idx], False) if P else ()
            nlp, _, entropy, mu, sigma = ot.forward_train(orc.p, obs, priv, d["actions"][idx], n_pl, n_l, *extra)
            k32, k64 = approx_kl(nlp, d["neglogpacs"][idx])
            peek_kl = ot.policy_kl(mu, sigma, d["mus"][idx], d["sigmas"][idx])
        out["approx32"].append(k32.item())
        out["approx64"].append(k64.item())
        out["step_kls"].append(peek_kl.item())
        out["entropies"].append(entropy.mean().item())
        ep_kls.append(peek_kl)
        if k32.item() > 1.5 * thr:                     # :578-581: the break, before zero_grad
            orc.rms_obs.update(d["obses"][idx])        # :521-522 precede the check
            orc.rms_priv.update(d["priv_info"][idx])
            out["stop"], out["idx_stop"] = s, idx.clone()
            end_of_mini_epoch()
            break
        st = orc.update(start_step=s, max_steps=1)
        assert torch.equal(peek_kl, st["step_kls"][0]), "the driver's peek is not the oracle's step"
        assert torch.equal(entropy.mean(), st["entropies"][0])
        out["step_lr"].append(lr)
        for k in ("a_losses", "c_losses", "b_losses"):
            out[k].append(st[k][0].item())
        if i == n_mb - 1:
            end_of_mini_epoch()
    out["params"] = orc.flat_params().numpy()
    adam = orc.adam_state()
    out["adam_m"] = torch.cat([m.reshape(-1) for m, _ in adam.values()]).numpy()
    out["adam_v"] = torch.cat([v.reshape(-1) for _, v in adam.values()]).numpy()
    for k, r in (("rms_obs", orc.rms_obs), ("rms_priv", orc.rms_priv)):
        out[k] = (r.mean.numpy().copy(), r.var.numpy().copy(), float(r.count))
    out["mus"], out["sigmas"] = d["mus"].numpy().copy(), d["sigmas"].numpy().copy()
    for k in ("approx32", "approx64", "step_kls", "entropies", "a_losses", "c_losses", "b_losses", "kls", "lrs", "kl_seen",
              "step_lr"):
        out[k] = np.array(out[k], dtype=np.float64)
    return out


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """The oracle run of a case, computed once per process (read-only for its users)."""
    return drive_oracle(name)


def assert_margins(name, ref=None):
    """The 10 % condition on the oracle's own estimator sequence, the expected stop step, and (combined case) the rate
    decisions' margin."""
    ref = case_oracle(name) if ref is None else ref
    limit = 1.5 * ref["thr"]
    assert ref["stop"] == CASES[name]["stop"], (name, ref["stop"], ref["approx32"])
    n = len(ref["approx32"])
    before = ref["approx32"][:n - 1] if ref["stop"] is not None else ref["approx32"]
    assert np.all(before <= (1.0 - MARGIN) * limit), (name, before.max(), limit)
    if ref["stop"] is not None:
        assert ref["approx32"][-1] >= (1.0 + MARGIN) * limit, (name, ref["approx32"][-1], limit)
    for kl in ref["kl_seen"]:
        assert L.boundary_distance(kl, ref["thr"]) >= L.MARGIN, (name, kl, ref["thr"])


def estimator_atol(ref):
    """A = 8 x the largest |fp32 CPU - float64| over the case's steps (the factor covers a device expf that differs
    from libm by an ulp of values near 1 before averaging)."""
    return 8.0 * float(np.abs(ref["approx32"] - ref["approx64"]).max())
