"""Device-side state of the teacher PPO update and its calls into libigi_hip.so.

``TeacherEngine`` owns the HBM-resident arenas (flat parameters / gradients / Adam moments, packed
fp64 normaliser states, prepared per-update arrays, workspace) and exposes the C-ABI entry points
as methods.  The reference-shaped classes (algo.ppo.frozen_ppo.PPO, ExperienceBuffer,
ActorCriticSplit, RunningMeanStd) hold *views* into these tensors.

torch is used here for device memory, streams and (multi-GPU) torch.distributed only.
"""
import ctypes as C
import os
from collections import OrderedDict

import torch

from . import _lib, ops

# hyper-parameter defaults: cfg/train/FactoryTaskInsertionTactilePPOv2.yaml:28-45, Adam defaults
DEFAULT_HP = dict(gamma=0.99, tau=0.95, lr=2.5e-4, beta1=0.9, beta2=0.999, adam_eps=1e-8, e_clip=0.2,
                  critic_coef=4.0, entropy_coef=0.0, bounds_loss_coef=1e-4, grad_norm=1.0,
                  truncate_grads=True, rms_eps=1e-5, normalize_value=True)

ROLLOUT_KEYS = ("obses", "priv_info", "rewards", "values", "neglogpacs", "dones", "actions", "mus",
                "sigmas", "last_values")


CONTACT_HIDDEN = 32   # ContactAE hidden width (models_split.py:46-47)
CONTACT_NAMES = ("contact_ae.contact_enc_mlp.0.weight", "contact_ae.contact_enc_mlp.0.bias",
                 "contact_ae.contact_enc_mlp.2.weight", "contact_ae.contact_enc_mlp.2.bias",
                 "contact_ae.contact_dec_mlp.0.weight", "contact_ae.contact_dec_mlp.0.bias",
                 "contact_ae.contact_dec_mlp.2.weight", "contact_ae.contact_dec_mlp.2.bias")


def teacher_param_names(n_priv_layers, n_layers, contacts=False, shared_parameters=False):
    """ActorCriticSplit.state_dict() key order (models_split.py:73-106); contact_ae between env_mlp
    and actor_mlp when the teacher has ground-truth contacts (models_split.py:81-84); no critic_mlp with a shared
    trunk (models_split.py:100-102)."""
    names = ["sigma"]
    for i in range(n_priv_layers):
        names += [f"env_mlp.mlp.{2 * i}.weight", f"env_mlp.mlp.{2 * i}.bias"]
    if contacts:
        names += list(CONTACT_NAMES)
    for net in ("actor_mlp",) if shared_parameters else ("actor_mlp", "critic_mlp"):
        for i in range(n_layers):
            names += [f"{net}.mlp.{2 * i}.weight", f"{net}.mlp.{2 * i}.bias"]
    names += ["value.weight", "value.bias", "mu.weight", "mu.bias"]
    return names


def teacher_param_shapes(obs_dim, priv_dim, act_dim, units, priv_units, contact_points=0, contact_emb=0,
                         only_contact=False, shared_parameters=False):
    shapes = OrderedDict()
    shapes["sigma"] = (act_dim,)
    d = priv_dim
    for i, u in enumerate(priv_units):
        shapes[f"env_mlp.mlp.{2 * i}.weight"] = (u, d)
        shapes[f"env_mlp.mlp.{2 * i}.bias"] = (u,)
        d = u
    trunk_in = obs_dim + priv_units[-1]
    if contact_points:
        H, P, E = CONTACT_HIDDEN, contact_points, contact_emb
        for k, shp in zip(CONTACT_NAMES, ((H, P), (H,), (E, H), (E,), (H, E), (H,), (P, H), (P,))):
            shapes[k] = shp
        if not only_contact:
            trunk_in += E
    for net in ("actor_mlp",) if shared_parameters else ("actor_mlp", "critic_mlp"):
        d = trunk_in
        for i, u in enumerate(units):
            shapes[f"{net}.mlp.{2 * i}.weight"] = (u, d)
            shapes[f"{net}.mlp.{2 * i}.bias"] = (u,)
            d = u
    shapes["value.weight"] = (1, units[-1])
    shapes["value.bias"] = (1,)
    shapes["mu.weight"] = (act_dim, units[-1])
    shapes["mu.bias"] = (act_dim,)
    return shapes


LR_SCHEDULES = ("fixed", "adaptive")


def lr_schedule_id(name):
    """train.ppo.lr_schedule -> igi_teacher_cfg.lr_schedule (None = absent = fixed)."""
    name = "fixed" if name is None else name
    if name not in LR_SCHEDULES:
        raise ValueError(f"lr_schedule {name!r}: supported schedules are {' and '.join(map(repr, LR_SCHEDULES))}")
    return LR_SCHEDULES.index(name)


def adaptive_lr_rule(lr, kl, kl_threshold, lr_min=1e-6, lr_max=1e-2):
    """The decision k_lr_schedule takes on the device, restated in Python doubles (= AdaptiveScheduler.update,
    frozen_ppo.py:864-877): strict inequalities, clamps applied to the moved rate only."""
    new = lr
    if kl > 2.0 * kl_threshold:
        new = max(lr / 1.5, lr_min)
    if kl < 0.5 * kl_threshold:
        new = min(lr * 1.5, lr_max)
    return new


def parse_kl_early_stop(value):
    """train.ppo.kl_early_stop -> bool (None = absent = off); ValueError for anything that is not a boolean -- a string
    such as "yes" or a number would otherwise switch it on silently."""
    if value is None:
        return False
    if isinstance(value, bool):
        return value
    raise ValueError(f"kl_early_stop {value!r}: expected True or False")


def kl_stop_rule(approx_kl, kl_threshold):
    """The decision the statistics block takes on the device, restated in Python doubles (frozen_ppo.py:578 made live):
    the fp32 estimator, widened, strictly above 1.5 * kl_threshold."""
    return float(approx_kl) > 1.5 * float(kl_threshold)


def slice_update_lists(stats, mini_epochs, n_mb, stop_step):
    """The reference's per-update lists from the (steps, 8) statistics rows when optimizer step ``stop_step`` stopped
    the update (frozen_ppo.py:571-581, 611-630 with the break live); ``None`` = it ran through.  At a stop at step
    s = e * n_mb + i the losses and grad norms have s entries (appended behind the break), the entropies s + 1 (appended
    in front of it), and the KL list e + 1: whole mini-epochs' means and, last, the mean over steps (e, 0 .. i).  Rows
    behind s are never read.  Returns a_losses, c_losses, b_losses, entropies, kls, grad_norms as lists of 0-d tensors."""
    total = mini_epochs * n_mb
    s = total if stop_step is None else int(stop_step)
    if not 0 <= s <= total or (stop_step is not None and s == total):
        raise ValueError(f"stop_step {stop_step}: expected None or 0 .. {total - 1}")
    n_ent = s if stop_step is None else s + 1
    rows = stats[:total]
    a_losses, c_losses, b_losses = (list(rows[:s, j].unbind()) for j in (0, 1, 2))
    entropies, grad_norms = list(rows[:n_ent, 3].unbind()), list(rows[:s, 6].unbind())
    kls = [rows[e * n_mb:min((e + 1) * n_mb, n_ent), 4].mean() for e in range((n_ent + n_mb - 1) // n_mb)]
    return a_losses, c_losses, b_losses, entropies, kls, grad_norms


def make_cfg(obs_dim, priv_dim, act_dim, units, priv_units, num_envs, horizon, mini_epochs, contact_points=0,
             contact_emb=0, only_contact=False, lr_schedule="fixed", kl_threshold=0.008, lr_min=1e-6, lr_max=1e-2,
             shared_parameters=False, **hp):
    """shared_parameters: one actor-critic trunk, value = value(actor_mlp(x)) (train.ppo.shared_parameters; not with
    contacts).  contact_points > 0: the teacher with ground-truth contacts (task.env.compute_contact_gt; num_points P,
    contact_mlp.units[-1] = contact_emb, train.ppo.only_contact).  lr_schedule "adaptive": the KL-adaptive learning
    rate scheduled on the device (kl_threshold, lr_min, lr_max as rl_games' AdaptiveScheduler); "fixed" leaves the four
    schedule fields zero, whatever the other three arguments say."""
    h = dict(DEFAULT_HP)
    h.update(hp)
    sched = lr_schedule_id(lr_schedule)
    if sched and not (float(kl_threshold) > 0 and 0 < float(lr_min) <= float(lr_max)):
        raise ValueError("the adaptive schedule needs kl_threshold > 0 and 0 < lr_min <= lr_max")
    if shared_parameters and contact_points:
        raise NotImplementedError("shared_parameters with compute_contact_gt is not supported")
    if contact_points:
        if not 1 <= contact_emb <= 32:
            raise ValueError(f"contact embedding width {contact_emb}: 1 .. 32 supported")
        if only_contact and contact_emb != priv_units[-1]:
            raise NotImplementedError("only_contact needs contact_mlp.units[-1] == priv_mlp_units[-1] "
                                      "(the reference sizes the trunk input as obs + priv latent)")
    elif contact_emb or only_contact:
        raise ValueError("contact_emb / only_contact need contact_points > 0")
    if len(units) > _lib.IGI_MAX_LAYERS or len(priv_units) > _lib.IGI_MAX_LAYERS:
        raise ValueError(f"at most {_lib.IGI_MAX_LAYERS} layers per MLP are supported")
    c = _lib.TeacherCfg()
    c.obs_dim, c.priv_dim, c.act_dim = obs_dim, priv_dim, act_dim
    c.n_priv_layers, c.n_layers = len(priv_units), len(units)
    for i, u in enumerate(priv_units):
        c.priv_units[i] = int(u)
    for i, u in enumerate(units):
        c.units[i] = int(u)
    c.num_envs, c.horizon, c.mini_epochs = num_envs, horizon, mini_epochs
    c.shared_parameters = int(bool(shared_parameters))
    c.gamma, c.tau = float(h["gamma"]), float(h["tau"])
    c.lr, c.beta1, c.beta2, c.adam_eps = float(h["lr"]), float(h["beta1"]), float(h["beta2"]), float(h["adam_eps"])
    c.e_clip, c.critic_coef = float(h["e_clip"]), float(h["critic_coef"])
    c.entropy_coef, c.bounds_loss_coef = float(h["entropy_coef"]), float(h["bounds_loss_coef"])
    c.grad_norm = float(h["grad_norm"]) if h["truncate_grads"] else 0.0
    c.rms_eps = float(h["rms_eps"])
    c.contact_points, c.contact_emb, c.only_contact = int(contact_points), int(contact_emb), int(bool(only_contact))
    if sched:
        c.lr_schedule, c.kl_threshold, c.lr_min, c.lr_max = sched, float(kl_threshold), float(lr_min), float(lr_max)
    return c, h


def param_layout(cfg):
    """(padded length, [(offset, size)] per tensor in state_dict order) from the library."""
    L = _lib.lib()
    n = L.igi_teacher_param_offsets(C.byref(cfg), None, None, 0)
    if n < 0:
        _lib.check(n, "igi_teacher_param_offsets")
    off = (C.c_int64 * n)()
    sz = (C.c_int64 * n)()
    L.igi_teacher_param_offsets(C.byref(cfg), off, sz, n)
    total = L.igi_teacher_param_count(C.byref(cfg))
    return int(total), [(int(off[i]), int(sz[i])) for i in range(n)]


class TeacherEngine:
    def __init__(self, num_envs, horizon, mini_epochs, units=(512, 256, 128), priv_units=(256, 128, 8),
                 obs_dim=15, priv_dim=64, act_dim=6, device="cuda:0", perm=None, contact_points=0, contact_emb=0,
                 only_contact=False, lr_schedule="fixed", kl_threshold=0.008, lr_min=1e-6, lr_max=1e-2,
                 kl_early_stop=False, shared_parameters=False, **hp):
        """shared_parameters: one trunk for actor and critic (train.ppo.shared_parameters; ``engine.shared_parameters``).
        kl_early_stop: stop an update at the first optimizer step whose approx_kl exceeds 1.5 * kl_threshold, decided
        on the device (``stop_step``, ``steps_applied``, ``approx_kl()``); data parallel: from the rank-mean estimator."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TeacherEngine needs a HIP device (there is no CPU path)")
        self.L = _lib.lib()
        self.cfg, self.hp = make_cfg(obs_dim, priv_dim, act_dim, units, priv_units, num_envs, horizon,
                                     mini_epochs, contact_points=contact_points, contact_emb=contact_emb,
                                     only_contact=only_contact, lr_schedule=lr_schedule, kl_threshold=kl_threshold,
                                     lr_min=lr_min, lr_max=lr_max, shared_parameters=shared_parameters, **hp)
        self.shared_parameters = bool(self.cfg.shared_parameters)
        self.adaptive_lr = bool(self.cfg.lr_schedule)
        self.kl_early_stop = parse_kl_early_stop(kl_early_stop)
        self._kl_threshold = float(kl_threshold)
        if self.kl_early_stop and not self._kl_threshold > 0:
            raise ValueError("kl_early_stop needs kl_threshold > 0")
        self.contact_points, self.contact_emb, self.only_contact = int(contact_points), int(contact_emb), bool(only_contact)
        self.N, self.T, self.E = num_envs, horizon, mini_epochs
        self.B = num_envs * horizon
        self.mb = self.B // mini_epochs
        self.n_mb = self.B // self.mb
        self.obs_dim, self.priv_dim, self.act_dim = obs_dim, priv_dim, act_dim
        self.units, self.priv_units = list(units), list(priv_units)
        self.shapes = teacher_param_shapes(obs_dim, priv_dim, act_dim, self.units, self.priv_units, contact_points,
                                           contact_emb, only_contact, self.shared_parameters)
        self.P, self.layout = param_layout(self.cfg)
        assert len(self.layout) == len(self.shapes)
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.params = torch.zeros(self.P, **f32)
        self.grads = torch.zeros(self.P, **f32)
        self.adam_m = torch.zeros(self.P, **f32)
        self.adam_v = torch.zeros(self.P, **f32)
        self._adam_t, self._enqueued, self._stop_words = 0, None, None
        self.rms_obs = self._fresh_rms(obs_dim)
        self.rms_priv = self._fresh_rms(priv_dim)
        self.rms_value = self._fresh_rms(1)
        T, N, A = horizon, num_envs, act_dim
        self.returns_raw = torch.zeros(T, N, 1, **f32)
        self.advantages = torch.zeros(T, N, **f32)
        self.values_n = torch.zeros(T, N, 1, **f32)
        self.returns_n = torch.zeros(T, N, 1, **f32)
        self.mus_w = torch.zeros(T, N, A, **f32)
        self.sigmas_w = torch.zeros(T, N, A, **f32)
        self.stats = torch.zeros(mini_epochs * self.n_mb, _lib.IGI_STATS_PER_STEP, **f32)
        wbytes = self.L.igi_teacher_workspace_bytes(C.byref(self.cfg))
        if wbytes == 0:
            raise RuntimeError("igi_teacher_workspace_bytes rejected the configuration: "
                               + self.L.igi_last_error().decode())
        self.workspace = torch.zeros(wbytes, dtype=torch.uint8, device=dev)
        self.workspace_trial_ms = None      # see tune_workspace
        # adaptive schedule: [rate, exchange scratch, (kl, rate after) per mini-epoch] as doubles (igi_teacher_state.lr_state)
        self.lr_state = None
        if self.adaptive_lr:
            self.lr_state = torch.zeros(_lib.lr_state_doubles(mini_epochs), dtype=torch.float64, device=dev)
            self.lr_state[0] = self.cfg.lr
        # KL early stopping: [stop step (-1 = none), reserved, approx_kl per optimizer step] as 32-bit words (igi_kl_stop)
        self.stop_state = None
        if self.kl_early_stop:
            self.stop_state = torch.zeros(_lib.stop_state_words(mini_epochs * self.n_mb), dtype=torch.int32, device=dev)
            self.stop_state[0] = -1
        if perm is None:
            perm = torch.randperm(self.B, device=dev)          # experience.py:202, drawn once
        self.perm = perm.to(device=dev, dtype=torch.int64).contiguous()
        self._ro = None

    def _fresh_rms(self, d):
        s = torch.zeros(2 * d + 1, dtype=torch.float64, device=self.device)
        s[d:2 * d] = 1.0   # running_var = 1 (running_mean_std.py:45)
        s[2 * d] = 1.0     # count = 1     (running_mean_std.py:46)
        return s

    # ---- parameters --------------------------------------------------------------------------
    def param_views(self, flat=None):
        flat = self.params if flat is None else flat
        out = OrderedDict()
        for (name, shape), (off, size) in zip(self.shapes.items(), self.layout):
            out[name] = flat[off:off + size].view(shape)
        return out

    def load_params(self, state_dict):
        views = self.param_views()
        for k, v in views.items():
            v.copy_(state_dict[k].to(self.device, torch.float32))

    def packed(self, flat=None):
        """Unpadded concatenation in state_dict order (what the reference's torch.cat produces)."""
        return torch.cat([v.reshape(-1) for v in self.param_views(flat).values()])

    # ---- native calls (torch.ops.mi355ppo.*: schema-checked, device-guarded; see ops.py) -------------------------
    def state_list(self):
        """The sixteen tensors of struct igi_teacher_state, in field order (+ lr_state under the adaptive schedule)."""
        st = [getattr(self, k) for k in ops.STATE_FIELDS]
        return st + [self.lr_state] if self.adaptive_lr else st

    # ---- KL early stopping ---------------------------------------------------------------------
    @property
    def kl_threshold(self):
        """The ONE threshold: the early stop compares against 1.5 x it and, under ``lr_schedule="adaptive"``, the
        scheduler against 0.5 x and 2 x it -- setting it here sets the cfg's field too."""
        return self._kl_threshold

    @kl_threshold.setter
    def kl_threshold(self, thr):
        thr = float(thr)
        if (self.kl_early_stop or self.adaptive_lr) and not thr > 0:
            raise ValueError("kl_threshold must be > 0")
        self._kl_threshold = thr
        if self.adaptive_lr:
            self.cfg.kl_threshold = thr

    def _stop_record(self):
        """The stop record of the last update as CPU int32 words, read from the device ONCE per update (the read
        synchronises; trainers make it next to the statistics read): ``stop_step``, ``steps_applied``, ``approx_kl()``
        and ``adam_t`` all derive from this one copy.  Enqueueing anything that writes the record drops the copy."""
        if self._stop_words is None:
            self._stop_words = self.stop_state.cpu()
        return self._stop_words

    @property
    def adam_t(self):
        """Optimizer steps applied so far.  After an update with ``kl_early_stop`` the host does not know it until it has
        read the stop record: the first look after such an update uses ``_stop_record``."""
        if self._enqueued is not None:
            base, n = self._enqueued
            s = int(self._stop_record()[0])
            self._adam_t, self._enqueued = base + (s if 0 <= s < n else n), None
        return self._adam_t

    @adam_t.setter
    def adam_t(self, t):
        self._adam_t, self._enqueued = int(t), None

    @property
    def stop_step(self):
        """The optimizer step that stopped the last update (it and every later one were not applied), or None when the
        update ran through -- always None without ``kl_early_stop``."""
        if not self.kl_early_stop:
            return None
        s = int(self._stop_record()[0])
        return s if s >= 0 else None

    @property
    def steps_applied(self):
        """Optimizer steps the last update applied: ``stop_step``, or all E * n_mb of them."""
        s = self.stop_step
        return self.E * self.n_mb if s is None else s

    def approx_kl(self):
        """The estimator mean((exp(d) - 1) - d), d = neglogp_new - neglogp_old, of every optimizer step the last update
        evaluated -- ``stop_step`` + 1 of them, or all -- as a float32 CPU tensor (data parallel: the rank mean)."""
        if not self.kl_early_stop:
            raise RuntimeError("approx_kl: the engine was built without kl_early_stop")
        w = self._stop_record()
        s = int(w[0])
        return w[2:].view(torch.float32)[:(s + 1 if s >= 0 else self.E * self.n_mb)].clone()

    def _stop_args(self):
        """(state list, icfg, fcfg) of the three ops that take the early-stopping tail."""
        icfg, fcfg = self._cfg_args()
        if not self.kl_early_stop:
            return self.state_list(), icfg, fcfg
        self._stop_words = None          # what is about to be enqueued rewrites the record
        icfg, fcfg, st = ops.pack_stop(icfg, fcfg, self.state_list(), self.kl_threshold, self.stop_state)
        return st, icfg, fcfg

    def _no_stop_dp(self, what):
        if self.kl_early_stop:
            raise RuntimeError(f"{what}: with kl_early_stop the ranks exchange the estimator between the norm kernel and "
                               "the Adam tail, which the step-wise two-phase loop has no place for: use update_dp / "
                               "update_dp_native")

    # ---- learning rate -------------------------------------------------------------------------
    @property
    def lr(self):
        """The rate the next optimizer step uses.  Adaptive schedule: read from the device (synchronises)."""
        return float(self.lr_state[0].item()) if self.adaptive_lr else float(self.cfg.lr)

    def set_lr(self, lr):
        """Fixed: cfg.lr.  Adaptive: an asynchronous fill of the device double on the current stream (no host sync)."""
        if self.adaptive_lr:
            self.lr_state[0:1].fill_(float(lr))
        else:
            self.cfg.lr = float(lr)

    def lr_history(self):
        """Adaptive schedule: the last update's record as an (E, 2) float64 CPU tensor -- per mini-epoch the mean KL as
        the scheduler compared it and the rate after its decision (synchronises)."""
        if not self.adaptive_lr:
            raise RuntimeError("lr_history: the engine runs the fixed schedule")
        return self.lr_state[2:].cpu().reshape(self.E, 2)

    def _cfg_args(self):
        """The packed igi_teacher_cfg, rebuilt from the struct on every call: trainers mutate ``cfg.lr`` and
        ``ExperienceBuffer.computer_return(last_values, gamma, tau)`` mutates ``cfg.gamma`` / ``cfg.tau``
        (experience.py:242), so no field may be cached.  32 scalars -- noise next to one native call."""
        return ops.pack_cfg(self.cfg)

    def set_rollout(self, ro):
        """ro: dict of time-major device tensors (ROLLOUT_KEYS, + "contacts" (T, N, P) for a contact teacher); kept
        referenced, not copied."""
        keep = []
        for k in ROLLOUT_KEYS + (("contacts",) if self.contact_points else ()):
            t = ro[k]
            want = torch.uint8 if k == "dones" else torch.float32
            if t.device != self.device or t.dtype != want or not t.is_contiguous():
                t = t.to(device=self.device, dtype=want).contiguous()
            keep.append(t)
        self._ro = keep

    def tune_workspace(self, trials=None):
        """Pick the workspace ALLOCATION the update runs fastest on.  Why: the env_mlp backward level takes 39 us per
        optimizer step on some workspace allocations and 40 - 48 us on others of the same size and alignment -- constant for
        the life of the allocation (tools/probes/env_level_time.py), no other kernel of the step affected, and only in the
        context of a whole step (the launch repeated on its own, with its operands cache-resident, runs the fast figure on
        every allocation; identical TLB / L2 counters: DESIGN.md section 7) -- up to 2 % of the update.  So, once, with a
        rollout set: run ONE whole update on each of ``trials`` candidate workspaces (all alive at once, else the caching
        allocator hands the same block back), sum its kernels' durations from the library's dispatch timestamps, keep the
        fastest candidate, and put every state tensor and the step counter back exactly as they were (the workspace holds
        nothing that outlives an update).  No collectives: in a multi-rank job every rank tunes on its own.  Costs ``trials`` + 1
        updates of wall time; ``IGI_WS_TRIALS`` (default 6; 1 = off) sets the default.  Returns the per-candidate update
        durations in ms (first entry = the allocation the engine was built with), also kept in ``workspace_trial_ms``."""
        trials = int(os.environ.get("IGI_WS_TRIALS", "6")) if trials is None else int(trials)
        if trials <= 1 or self._ro is None or self.device.type != "cuda":
            return None
        keys = [k for k in ops.STATE_FIELDS if k not in ("perm", "workspace")] + (["lr_state"] if self.adaptive_lr else []) \
            + (["stop_state"] if self.kl_early_stop else [])
        snap = {k: getattr(self, k).clone() for k in keys}
        t0, cfg0 = self.adam_t, (self.cfg.gamma, self.cfg.tau, self.cfg.lr)
        cands = [self.workspace]
        for _ in range(trials - 1):
            try:
                cands.append(torch.zeros_like(self.workspace))
            except RuntimeError:          # out of memory: choose among what there is
                break
        if len(cands) < 2:
            return None
        times = []
        try:
            with torch.cuda.device(self.device):
                self.prepare()
                self.update()            # untimed: the first update of a process also pays code loading and clock ramp-up
                for w in cands:
                    for k in keys:
                        getattr(self, k).copy_(snap[k])
                    self.adam_t, self.workspace = t0, w
                    self.prepare()
                    torch.cuda.synchronize()
                    _lib.prof_enable(True)
                    try:
                        self.update()
                        torch.cuda.synchronize()
                        classes = _lib.prof_read()
                    finally:
                        _lib.prof_enable(False)
                    times.append(round(sum(c["total_ms"] for c in classes), 4))
        finally:
            for k in keys:
                getattr(self, k).copy_(snap[k])
            self.adam_t, self._stop_words = t0, None
            self.cfg.gamma, self.cfg.tau, self.cfg.lr = cfg0
            self.workspace = cands[0]
        if len(times) == len(cands) and all(t > 0 for t in times):
            self.workspace = cands[min(range(len(times)), key=times.__getitem__)]
            self.workspace_trial_ms = times
        return self.workspace_trial_ms

    def prepare(self, ro=None):
        """computer_return + prepare_training + value normalisation (experience.py:242-263;
        frozen_ppo.py:717-725)."""
        if ro is not None:
            self.set_rollout(ro)
        torch.ops.mi355ppo.gae_advnorm(self._ro, self.state_list(), *self._cfg_args(), bool(self.hp["normalize_value"]))

    def fwd_bwd(self, mb_index, slot):
        torch.ops.mi355ppo.ppo_minibatch_fwd_bwd(self._ro, *self._stop_args(), mb_index, slot, -1)

    def fwd_bwd_phase(self, mb_index, slot, phase):
        """Phase 0: down to dZ of the first trunk layer (the EARLY gradient bucket is final); phase 1: latent + env_mlp
        backward and the first trunk layer's weight gradient (the LATE bucket is final).  See ``grad_buckets``."""
        self._no_stop_dp("fwd_bwd_phase")
        torch.ops.mi355ppo.ppo_minibatch_fwd_bwd(self._ro, self.state_list(), *self._cfg_args(), mb_index, slot, phase)

    @property
    def grad_buckets(self):
        """((early ranges), (late ranges)) of the flat gradient as (offset, length) pairs, empty ranges dropped:
        early = actor layers >= 1 | critic layers >= 1 + value + mu; late = sigma + env_mlp + actor layer 0 | critic
        layer 0 (igi_teacher_grad_buckets).  Shared trunk: one early range (actor layers >= 1 + value + mu) and one late."""
        off, ln = (C.c_int64 * 4)(), (C.c_int64 * 4)()
        n = self.L.igi_teacher_grad_buckets(C.byref(self.cfg), off, ln)
        if n != 4:
            _lib.check(n, "igi_teacher_grad_buckets")
        r = [(int(off[i]), int(ln[i])) for i in range(4)]
        return tuple(x for x in r[:2] if x[1] > 0), tuple(x for x in r[2:] if x[1] > 0)

    def bucket_views(self):
        early, late = self.grad_buckets
        return [self.grads[o:o + n] for o, n in early], [self.grads[o:o + n] for o, n in late]

    def apply(self, slot, grad_scale=1.0):
        if self.kl_early_stop:
            # steps 0 .. slot of this update are enqueued; how many of them the device applied, the stop word says
            base = self.adam_t if slot == 0 or self._enqueued is None else self._enqueued[0]
            torch.ops.mi355ppo.ppo_clip_adam(*self._stop_args(), slot, base + slot + 1, float(grad_scale))
            self._enqueued = (base, slot + 1)
            return
        self.adam_t += 1
        torch.ops.mi355ppo.ppo_clip_adam(self.state_list(), *self._cfg_args(), slot, self.adam_t, float(grad_scale))

    def update(self):
        """mini_epochs x n_minibatch optimizer steps enqueued back to back (frozen_ppo.py:508-640).
        Returns the (E*n_mb, 8) stats tensor (device; no host sync here)."""
        t0 = self.adam_t
        torch.ops.mi355ppo.ppo_update(self._ro, *self._stop_args(), t0)
        self._count_update(t0)
        return self.stats

    def _count_update(self, t0):
        """A whole update was enqueued from step count t0: with kl_early_stop the first look at adam_t resolves it."""
        if self.kl_early_stop:
            self._enqueued = (t0, self.E * self.n_mb)
        else:
            self.adam_t = t0 + self.E * self.n_mb

    def update_dp(self, all_reduce, world_size, all_reduce_async=None):
        """Same loop with a gradient all-reduce between backward and the optimizer
        (frozen_ppo.py:586-603): SUM over ranks, the 1/world is folded into the Adam kernel.

        ``all_reduce_async(t) -> work`` (``dist.all_reduce(t, async_op=True)``) enables the overlapped
        schedule: the early bucket (trunk layers >= 1 and the heads, 81 % of the bytes, two ranges) is reduced on the
        collective's stream while the latent / env_mlp backward still runs on the compute stream; ``work.wait()`` only orders the
        streams, the host never blocks.  Either way the whole update is ONE native call
        (igi_teacher_update_dp); the library calls back between the stages of a step."""
        early, late = self.bucket_views()
        pending = []
        kl_view = self.lr_state.view(torch.float32)[2:3] if self.adaptive_lr else None   # the float of lr_state[1]
        akl_view = self.stop_state.view(torch.float32)[1:2] if self.kl_early_stop else None   # the float of stop_state[1]

        def reducer(bucket, step):
            if bucket == 4:                   # KL early stopping: the step's estimator, one float, in stream order
                if all_reduce_async is not None:
                    all_reduce_async(akl_view).wait()
                else:
                    all_reduce(akl_view)
            elif bucket == 3:                   # adaptive schedule: the mini-epoch's KL, one float, in stream order
                if all_reduce_async is not None:
                    all_reduce_async(kl_view).wait()
                else:
                    all_reduce(kl_view)
            elif bucket == 2:
                for w in pending:
                    if w is not None:
                        w.wait()
                pending.clear()
            elif all_reduce_async is not None:
                for view in (early if bucket == 0 else late):
                    pending.append(all_reduce_async(view))
            elif bucket == 1:                 # serial schedule: everything after backward, like the reference
                all_reduce(self.grads)

        h = ops.register_reducer(reducer)
        try:
            t0 = self.adam_t
            torch.ops.mi355ppo.ppo_update_dp(self._ro, *self._stop_args(), t0, 1.0 / world_size, h)
        finally:
            ops.unregister_reducer(h)
        self._count_update(t0)
        return self.stats

    def update_dp_native(self, comm, overlap=True, want_stats_sum=False):
        """The data-parallel update with the gradient exchange issued by the library over its own RCCL communicator
        (``utils.dist.NativeComm``): one native call, no callback -- igi_teacher_update_dp_rccl.  ``want_stats_sum``:
        also returns the per-step statistics summed over the ranks (one collective per update)."""
        stats_sum = torch.empty_like(self.stats) if want_stats_sum else None
        t0 = self.adam_t
        torch.ops.mi355ppo.ppo_update_dp_rccl(self._ro, *self._stop_args(), t0, int(comm.handle), bool(overlap), stats_sum)
        self._count_update(t0)
        return (self.stats, stats_sum) if want_stats_sum else self.stats

    def infer(self, obs, priv, want_latent=False, normalize=True):
        """model_act forward without sampling (models_split.py:120-164).  normalize=True: raw inputs,
        normalised with the current running stats (eval mode); False: inputs already processed.
        Returns (mu, value_normalised[, latent])."""
        obs = obs.to(self.device, torch.float32).contiguous()
        priv = priv.to(self.device, torch.float32).contiguous()
        mu, val, lat = torch.ops.mi355ppo.actor_critic_infer(self.state_list(), *self._cfg_args(), obs, priv,
                                                              bool(normalize), bool(want_latent))
        return (mu, val, lat) if want_latent else (mu, val)

    def actor_latent(self, obs, latent, save=False):
        """The frozen actor on ``cat(obs, latent)`` (act_inference / act_with_grad with a student latent): obs normalised
        (rows, obs_dim), latent (rows, the teacher's extrinsic width), both fp32 and contiguous on the engine's device.
        Returns (mu, saved): ``saved`` holds the actor's activations for ``actor_latent_backward`` when ``save``."""
        return torch.ops.mi355ppo.actor_latent_fwd(self.state_list(), *self._cfg_args(), obs, latent, bool(save))

    def actor_latent_backward(self, saved, dmu):
        """d/d latent from ``actor_latent(..., save=True)``'s activations and d/d mu; the teacher's weights get nothing."""
        return torch.ops.mi355ppo.actor_latent_bwd(self.state_list(), *self._cfg_args(), saved, dmu)

    def infer_contacts(self, obs, priv, contacts, want_latent=False, normalize=True):
        """``infer`` for a contact teacher: contacts (rows, P) raw; the latent is latent_gt = [priv latent | contact
        embedding] (models_split.py:172-177)."""
        obs = obs.to(self.device, torch.float32).contiguous()
        priv = priv.to(self.device, torch.float32).contiguous()
        contacts = contacts.to(self.device, torch.float32).contiguous()
        mu, val, lat = torch.ops.mi355ppo.actor_critic_infer_contacts(self.state_list(), *self._cfg_args(), obs, priv,
                                                                       contacts, bool(normalize), bool(want_latent))
        return (mu, val, lat) if want_latent else (mu, val)

    # ---- reference-shaped accessors ------------------------------------------------------------
    def env_major(self, x):
        """(T,N,...) -> (N*T,...) like experience.py:39-46 (a copy; off the hot path)."""
        s = x.shape
        return x.transpose(0, 1).reshape(s[0] * s[1], *s[2:])

    def rms_dict(self, packed):
        d = (packed.numel() - 1) // 2
        return dict(running_mean=packed[:d], running_var=packed[d:2 * d], count=packed[2 * d])
