"""Teacher network with the reference's interface (algo/models/models_split.py:21-250):
``MLP``, ``layer_init``, ``ActorCriticSplit`` with ``act / full_act / act_inference / act_with_grad /
actor_critic / forward`` and the same state_dict keys, shapes and initialisation.

All parameters are views into ONE flat fp32 vector whose layout the HIP library defines
(igi_teacher_param_offsets: state_dict order, tensors 16-byte aligned); the fused PPO kernels read
and update that vector in place.  Forward evaluation runs through igi_teacher_infer (exact-fp32
MFMA); gradients of this network only exist inside the fused update (igi_teacher_fwd_bwd), so the
methods here return tensors without an autograd graph.
"""
import numpy as np
import torch
import torch.nn as nn

LOG_SQRT_2PI = 0.5 * float(np.log(2.0 * np.pi))


def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
    """models_split.py:21-24"""
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class MLP(nn.Module):
    """Linear+Tanh stack, tanh after every layer including the last (models_split.py:27-38).
    Container for parameters; evaluated by the fused kernels."""

    def __init__(self, units, input_size):
        super().__init__()
        layers = []
        for output_size in units:
            layers.append(layer_init(nn.Linear(input_size, output_size)))
            layers.append(nn.Tanh())
            input_size = output_size
        self.mlp = nn.Sequential(*layers)


class ContactAE(nn.Module):
    """Ground-truth contact autoencoder (models_split.py:41-55).  Its Linears keep torch's default initialisation;
    ``forward_enc`` runs the HIP contact encoder (csrc/contact.h).  The decoder is a state_dict member the trainer never
    evaluates (no reconstruction loss in the reference); ``forward_dec`` runs it on the native Linear op."""

    def __init__(self, input_size, embedding_size=16):
        nn.Module.__init__(self)
        self.embedding_size = embedding_size
        self.contact_enc_mlp = nn.Sequential(nn.Linear(input_size, 32), nn.ReLU(), nn.Linear(32, embedding_size),
                                             nn.Tanh())
        self.contact_dec_mlp = nn.Sequential(nn.Linear(embedding_size, 32), nn.ReLU(), nn.Linear(32, input_size))

    def forward_enc(self, x):
        if not x.is_cuda:
            raise RuntimeError("ContactAE runs on the HIP device only (no CPU fallback)")
        l1, l2 = self.contact_enc_mlp[0], self.contact_enc_mlp[2]
        packed = torch.cat([l1.weight.detach().reshape(-1), l1.bias.detach(), l2.weight.detach().reshape(-1),
                            l2.bias.detach()]).to(x.device, torch.float32)
        emb, _ = torch.ops.mi355ppo.contact_encoder_fwd(x.float().contiguous(), packed, self.embedding_size)
        return emb

    def forward_dec(self, x):
        from ...hip_linear import linear
        l1, l2 = self.contact_dec_mlp[0], self.contact_dec_mlp[2]
        h = linear(x, l1.weight.detach(), l1.bias.detach(), 'relu')
        return linear(h, l2.weight.detach(), l2.bias.detach())


class _ActorOnLatent(torch.autograd.Function):
    """mu = mu head(actor_mlp(cat(obs, latent))) on the native frozen-actor path (csrc/policy_fwd.h, k_actor_latent), with
    the data gradient back into the latent.  The observation and the teacher's weights get no gradient."""

    @staticmethod
    def forward(ctx, latent, obs, engine):
        mu, saved = engine.actor_latent(obs, latent, save=True)
        ctx.engine = engine
        ctx.save_for_backward(saved)
        return mu

    @staticmethod
    def backward(ctx, dmu):
        (saved,) = ctx.saved_tensors
        return ctx.engine.actor_latent_backward(saved, dmu.contiguous()), None, None


class ActorCriticSplit(nn.Module):
    def __init__(self, kwargs):
        nn.Module.__init__(self)
        actions_num = kwargs['actions_num']
        input_shape = kwargs['input_shape']
        mlp_input_shape = input_shape[0]
        self.units = list(kwargs['actor_units'])
        self.contact_info = kwargs.get('gt_contacts_info', False)
        self.only_contact = kwargs.get('only_contact', False)
        self.priv_mlp_units = list(kwargs['priv_mlp_units'])
        self.priv_info = kwargs['priv_info']
        self.priv_info_dim = kwargs['priv_info_dim']
        self.shared_parameters = kwargs.get('shared_parameters', False)
        self.vt_policy = kwargs.get('vt_policy', False)
        if not self.priv_info or self.vt_policy:
            # reference defaults: priv_info True, vt_policy hard-wired False (frozen_ppo.py:139) -- the configurations
            # on the hot path (separate critic or shared trunk; separate critic with or without ground-truth contacts)
            raise NotImplementedError("only priv_info=True without vt_policy is on the hot path")
        if self.shared_parameters and self.contact_info:
            raise NotImplementedError("shared_parameters with compute_contact_gt is not supported")
        self.obs_dim = mlp_input_shape
        self.actions_num = actions_num
        mlp_input_shape += self.priv_mlp_units[-1]
        self.env_mlp = MLP(units=self.priv_mlp_units, input_size=self.priv_info_dim)
        self.num_contact_points, self.contact_emb = 0, 0
        if self.contact_info:                         # models_split.py:78-84
            self.contact_mlp_units = list(kwargs['contacts_mlp_units'])
            self.num_contact_points = int(kwargs['num_contact_points'])
            self.contact_emb = int(self.contact_mlp_units[-1])
            if self.only_contact and self.contact_emb != self.priv_mlp_units[-1]:
                raise NotImplementedError("only_contact needs contact_mlp.units[-1] == priv_mlp_units[-1] (the reference "
                                          "sizes the trunk input as obs + priv latent and feeds it the contact embedding)")
            self.contact_ae = ContactAE(input_size=self.num_contact_points, embedding_size=self.contact_emb)
            if not self.only_contact:
                mlp_input_shape += self.contact_emb
        elif self.only_contact:
            raise NotImplementedError("only_contact without compute_contact_gt is not a configuration of the reference")
        self.actor_mlp = MLP(units=self.units, input_size=mlp_input_shape)
        if not self.shared_parameters:                # models_split.py:100-102: the value head then reads actor_mlp's output
            self.critic_mlp = MLP(units=self.units, input_size=mlp_input_shape)
        self.value = layer_init(torch.nn.Linear(self.units[-1], 1), std=1.0)
        self.mu = layer_init(torch.nn.Linear(self.units[-1], actions_num), std=0.01)
        self.sigma = nn.Parameter(torch.zeros(actions_num, requires_grad=True, dtype=torch.float32),
                                  requires_grad=True)
        for m in self.modules():                      # models_split.py:108-117
            if isinstance(m, nn.Linear) and getattr(m, 'bias', None) is not None:
                torch.nn.init.zeros_(m.bias)
        nn.init.constant_(self.sigma, 0)
        self._flat = None
        self._engine = None
        self._pack(torch.device("cpu"))

    # -- flat parameter vector --------------------------------------------------------------------
    def _layout(self):
        from ...teacher_native import make_cfg, param_layout
        cfg, _ = make_cfg(self.obs_dim, self.priv_info_dim, self.actions_num, self.units, self.priv_mlp_units,
                          2, 1, 1, **self.engine_kwargs())
        return param_layout(cfg)

    def _pack(self, device, flat=None):
        """(Re)build the flat vector on `device` and re-point every parameter at its slice."""
        total, layout = self._layout()
        params = list(self.parameters())           # registration order == state_dict order, sigma first
        order = [self.sigma] + [p for p in params if p is not self.sigma]
        assert len(order) == len(layout)
        if flat is None:
            flat = torch.zeros(total, dtype=torch.float32, device=device)
        for p, (off, size) in zip(order, layout):
            assert p.numel() == size
            view = flat[off:off + size].view(p.shape)
            view.copy_(p.data.to(flat.device))
            p.data = view
        self._flat = flat

    def bind_flat(self, flat):
        """Adopt the trainer engine's parameter vector (values are copied into it)."""
        self._pack(flat.device, flat)

    def contact_kwargs(self):
        """The contact fields of the teacher cfg (make_cfg / TeacherEngine keyword arguments)."""
        if not self.contact_info:
            return {}
        return dict(contact_points=self.num_contact_points, contact_emb=self.contact_emb,
                    only_contact=bool(self.only_contact))

    def engine_kwargs(self):
        """Everything of the teacher cfg that the network decides: the contact fields and the shared-trunk switch."""
        return dict(self.contact_kwargs(), shared_parameters=bool(self.shared_parameters))

    @property
    def flat_params(self):
        return self._flat

    def _apply(self, fn, recurse=True):
        new_flat = fn(self._flat)
        if new_flat is self._flat:          # .to(same device) / .float() / .cuda() on a cuda model: nothing moved,
            return self                     # the parameters stay views of the engine's vector
        self._pack(new_flat.device, new_flat)
        self._engine = None                 # a moved model gets a fresh inference engine on first use
        return self

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(state_dict, strict)   # copy_ into the views: layout preserved
        return out

    # -- evaluation ---------------------------------------------------------------------------------
    def attach_engine(self, engine):
        self._engine = engine

    def _infer_engine(self, device):
        if self._engine is None:
            from ...teacher_native import TeacherEngine
            eng = TeacherEngine(4096, 1, 1, units=self.units, priv_units=self.priv_mlp_units,
                                obs_dim=self.obs_dim, priv_dim=self.priv_info_dim, act_dim=self.actions_num,
                                device=device, **self.engine_kwargs())
            self.bind_flat_to(eng)
            self._engine = eng
        return self._engine

    def bind_flat_to(self, engine):
        engine.params.copy_(self._flat.to(engine.params.device))
        self.bind_flat(engine.params)

    def actor_critic(self, obs_dict, display=False):
        """models_split.py:166-232: returns (mu, logstd, value, extrin, extrin_gt)."""
        obs = obs_dict['obs']
        if not obs.is_cuda:
            raise RuntimeError("ActorCriticSplit runs on the HIP device only (no CPU fallback)")
        if 'latent' in obs_dict and obs_dict['latent'] is not None:
            return self._actor_critic_from_latent(obs_dict)
        eng = self._infer_engine(obs.device)
        if self.contact_info:                         # models_split.py:172-177: contacts go in raw
            mu, value, latent = eng.infer_contacts(obs, obs_dict['priv_info'], obs_dict['contacts'], want_latent=True,
                                                   normalize=False)
        else:
            mu, value, latent = eng.infer(obs, obs_dict['priv_info'], want_latent=True, normalize=False)
        logstd = mu * 0 + self.sigma.detach()
        return mu, logstd, value, None, latent

    def _actor_critic_from_latent(self, obs_dict):
        """models_split.py:187-216 with a student latent: the policy / value heads see ``cat(obs, latent)``
        instead of the privileged embedding.  Built from the native Linear+Tanh op so that autograd can carry a
        distillation loss on ``mu`` back into ``latent`` (ext_adapt.py:799-804); the teacher's weights are
        constants here (the student optimiser never steps them)."""
        from ...hip_linear import linear
        x = torch.cat([obs_dict['obs'], obs_dict['latent']], dim=-1)

        def trunk(mlp):
            h = x
            for layer in mlp.mlp:
                if isinstance(layer, nn.Linear):
                    h = linear(h, layer.weight.detach(), layer.bias.detach(), 'tanh')
            return h

        h_actor = trunk(self.actor_mlp)
        mu = linear(h_actor, self.mu.weight.detach(), self.mu.bias.detach())
        h_critic = h_actor if self.shared_parameters else trunk(self.critic_mlp)   # models_split.py:226-230
        value = linear(h_critic, self.value.weight.detach(), self.value.bias.detach())
        extrin_gt = None
        if 'priv_info' in obs_dict and obs_dict['priv_info'] is not None:
            with torch.no_grad():
                eng = self._infer_engine(x.device)
                if self.contact_info:
                    _, _, extrin_gt = eng.infer_contacts(obs_dict['obs'], obs_dict['priv_info'], obs_dict['contacts'],
                                                         want_latent=True, normalize=False)
                else:
                    _, _, extrin_gt = eng.infer(obs_dict['obs'], obs_dict['priv_info'], want_latent=True,
                                                normalize=False)
        logstd = mu * 0 + self.sigma.detach()
        return mu, logstd, value, obs_dict['latent'], extrin_gt

    @torch.no_grad()
    def act(self, obs_dict):
        """models_split.py:120-134 (sampling with the device generator)."""
        mu, logstd, value, _, _ = self.actor_critic(obs_dict)
        sigma = torch.exp(logstd)
        selected_action = mu + sigma * torch.randn_like(mu)
        return {
            'neglogpacs': self.neglogp(selected_action, mu, sigma),
            'values': value, 'actions': selected_action, 'mus': mu, 'sigmas': sigma,
        }

    @torch.no_grad()
    def full_act(self, obs_dict):
        """models_split.py:137-152"""
        mu, logstd, value, _, latent_gt = self.actor_critic(obs_dict)
        sigma = torch.exp(logstd)
        selected_action = mu + sigma * torch.randn_like(mu)
        return {
            'neglogpacs': self.neglogp(selected_action, mu, sigma),
            'values': value, 'actions': selected_action, 'mus': mu, 'sigmas': sigma, 'latent_gt': latent_gt,
        }

    @property
    def latent_width(self):
        """Columns behind the observation in the trunk's input: the privileged latent, [latent | contact embedding], or
        the embedding alone with only_contact (models_split.py:172-183) -- the width a student latent must have."""
        if not self.contact_info:
            return self.priv_mlp_units[-1]
        return self.contact_emb + (0 if self.only_contact else self.priv_mlp_units[-1])

    def _mu_from_latent(self, obs_dict):
        """mu of the frozen ACTOR on ``cat(obs, latent)`` -- what act_inference / act_with_grad keep of
        models_split.py:187-216 when a student latent is given; the value they throw away is not computed.  One
        k_actor_latent launch at the reference's layer sizes (csrc/policy_fwd.h), the actor's layers one by one otherwise;
        with grad enabled and a latent that requires it, autograd carries d/d mu back into the latent."""
        obs, latent = obs_dict['obs'], obs_dict['latent']
        if latent.dim() != 2 or latent.shape[-1] != self.latent_width:
            raise ValueError(f"latent of shape {tuple(latent.shape)}: width {latent.shape[-1] if latent.dim() else 0} given, "
                             f"this teacher's actor reads an extrinsic of width {self.latent_width} behind the observation")
        if not obs.is_cuda:
            raise RuntimeError("ActorCriticSplit runs on the HIP device only (no CPU fallback)")
        eng = self._infer_engine(obs.device)
        obs = obs.detach().to(torch.float32).contiguous()
        lat = latent.to(torch.float32).contiguous()
        if torch.is_grad_enabled() and lat.requires_grad:
            return _ActorOnLatent.apply(lat, obs, eng)
        return eng.actor_latent(obs, lat.detach(), save=False)[0]

    @torch.no_grad()
    def act_inference(self, obs_dict):
        """models_split.py:155-159"""
        if obs_dict.get('latent', None) is not None:
            return self._mu_from_latent(obs_dict), obs_dict['latent']
        mu, logstd, value, latent, latent_gt = self.actor_critic(obs_dict)
        latent = latent_gt if latent is None else latent
        return mu, latent

    def act_with_grad(self, obs_dict):
        """models_split.py:161-164.  With a ``latent`` entry the result carries an autograd graph back to it."""
        if obs_dict.get('latent', None) is not None:
            return self._mu_from_latent(obs_dict), obs_dict['latent']
        mu, logstd, value, latent, _ = self.actor_critic(obs_dict)
        return mu, latent

    @staticmethod
    def neglogp(x, mu, sigma):
        """-Normal(mu, sigma).log_prob(x).sum(1) (models_split.py:128)."""
        return (((x - mu) ** 2) / (2.0 * sigma ** 2) + torch.log(sigma) + LOG_SQRT_2PI).sum(dim=-1)

    @torch.no_grad()
    def forward(self, input_dict):
        """models_split.py:234-250 (evaluation only; training gradients live in the fused update)."""
        prev_actions = input_dict.get('prev_actions', None)
        mu, logstd, value, extrin, extrin_gt = self.actor_critic(input_dict)
        sigma = torch.exp(logstd)
        entropy = (0.5 + LOG_SQRT_2PI + torch.log(sigma)).sum(dim=-1)
        return {
            'prev_neglogp': torch.squeeze(self.neglogp(prev_actions, mu, sigma)),
            'values': value, 'entropy': entropy, 'mus': mu, 'sigmas': sigma,
            'extrin': extrin, 'extrin_gt': extrin_gt,
        }
