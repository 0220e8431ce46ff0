"""The teacher with ground-truth contacts (task.env.compute_contact_gt; models_split.py:41-55, 78-88, 166-183) on the GPU:
the contact encoder kernels against float64, the whole training step's gradient against a float64 restatement of the
reference's loss with ContactAE.forward_enc in the latent, inference, and the parameters that get no gradient (the
decoder always, env_mlp under only_contact) coming out of updates bit-unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HID = 32


def _enc64(C, W1, b1, W2, b2):
    h = torch.relu(C @ W1.T + b1)
    return torch.tanh(h @ W2.T + b2), h


def _encoder_vs_float64(P, rows, E):
    import isaacgyminsertion_amd.ops  # noqa: F401  (registers torch.ops.mi355ppo)
    g = torch.Generator().manual_seed(P * 7919 + rows + (0 if E == 8 else 104729 * E))
    C = (torch.rand(rows, P, generator=g) < 0.2).float()
    W1 = torch.randn(HID, P, generator=g) / np.sqrt(P)
    b1 = 0.1 * torch.randn(HID, generator=g)
    W2 = torch.randn(E, HID, generator=g) / np.sqrt(HID)
    b2 = 0.1 * torch.randn(E, generator=g)
    packed = torch.cat([W1.reshape(-1), b1, W2.reshape(-1), b2]).cuda()
    emb, hid = torch.ops.mi355ppo.contact_encoder_fwd(C.cuda(), packed, E)
    torch.cuda.synchronize()
    p64 = [t.double().requires_grad_(True) for t in (W1, b1, W2, b2)]
    e64, h64 = _enc64(C.double(), *p64)
    np.testing.assert_allclose(hid.cpu().numpy(), h64.detach().numpy(), atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(emb.cpu().numpy(), e64.detach().numpy(), atol=2e-6, rtol=1e-5)
    # backward from d(pre-tanh): dz = d(emb) * (1 - emb^2)
    dE = torch.randn(rows, E, generator=g)
    dz = (dE * (1 - emb.cpu() ** 2)).float()
    grads = torch.ops.mi355ppo.contact_encoder_bwd(C.cuda(), packed, hid, dz.cuda())
    torch.cuda.synchronize()
    (e64 * dE.double()).sum().backward()
    ref = torch.cat([p.grad.reshape(-1) for p in p64]).numpy()
    got = grads.cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=1e-4 * max(1.0, np.abs(ref).max()), rtol=1e-3)
    # deterministic
    again = torch.ops.mi355ppo.contact_encoder_bwd(C.cuda(), packed, hid, dz.cuda())
    assert torch.equal(again, grads)


# P: 4 / 36 take the float4 loader (P % 4 == 0) with a last chunk shorter than a lane half's 16 columns, 33 the scalar one
# with a one-column tail
@pytest.mark.parametrize("P", [1, 4, 33, 36, 37, 400, 1000])
@pytest.mark.parametrize("rows", [1, 77, 300, 4113])
def test_contact_encoder_matches_float64(P, rows):
    _encoder_vs_float64(P, rows, 8)


# the embedding axis (E = 8 is the test above): one column, one past a float4 / a quarter tile, the last and the full 32-row
# MFMA tile -- the e < E guards of both kernels.  Same bounds.
@pytest.mark.parametrize("E", [1, 9, 31, 32])
@pytest.mark.parametrize("P", [4, 37, 400])
@pytest.mark.parametrize("rows", [1, 77, 300])
def test_contact_encoder_embedding_widths_match_float64(rows, P, E):
    _encoder_vs_float64(P, rows, E)


# ---- the whole teacher step -------------------------------------------------------------------------------------
def _problem(N, T, units, priv_units, P, E, only_contact, seed=4321):
    from oracle import synth
    from isaacgyminsertion_amd.teacher_native import teacher_param_shapes
    base, ro, perm = synth.teacher_problem(N, T, units, priv_units, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    shapes = teacher_param_shapes(15, 64, 6, units, priv_units, P, E, only_contact)
    init = {}
    for k, shp in shapes.items():
        if k in base and tuple(base[k].shape) == tuple(shp):
            init[k] = base[k].clone().float()
        elif len(shp) == 2:
            init[k] = torch.randn(*shp, generator=g) / np.sqrt(shp[1])
        else:
            init[k] = 0.05 * torch.randn(*shp, generator=g)
    ro = dict(ro)
    ro["contacts"] = (torch.rand(T, N, P, generator=g) < 0.15).float()
    return init, ro, perm


def _engine(N, T, Ep, units, priv_units, P, E, only_contact, init, perm):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    eng = TeacherEngine(N, T, Ep, units=units, priv_units=priv_units, perm=perm, contact_points=P, contact_emb=E,
                        only_contact=only_contact)
    eng.load_params(init)
    return eng


def _ro_cuda(ro):
    return {k: v.cuda() for k, v in ro.items()}


def _step0_grad64(init, ro, perm, N, T, Ep, units, priv_units, only_contact):
    """Float64 restatement of optimizer step 0 (frozen_ppo.py:508-604) with the contact latent
    (models_split.py:166-183): gather, running-stat normalisation (contacts raw), forward, PPO losses, backward."""
    from oracle import teacher as ot
    orc = ot.TeacherOracle({k: v for k, v in init.items()}, perm, N, T, Ep, units, priv_units)
    d = orc.prepare({k: v for k, v in ro.items() if k != "contacts"})
    mb = N * T // Ep
    idx = perm[:mb]
    contacts = ot.env_major(ro["contacts"])[idx].double()
    obs = orc.rms_obs(d["obses"][idx], True).double()
    priv = orc.rms_priv(d["priv_info"][idx], True).double()
    p = {k: v.double().clone().requires_grad_(True) for k, v in init.items()}

    def mlp(prefix, n, x):
        for i in range(n):
            x = torch.tanh(torch.nn.functional.linear(x, p[f"{prefix}.mlp.{2 * i}.weight"], p[f"{prefix}.mlp.{2 * i}.bias"]))
        return x

    h = torch.relu(torch.nn.functional.linear(contacts, p["contact_ae.contact_enc_mlp.0.weight"],
                                              p["contact_ae.contact_enc_mlp.0.bias"]))
    ec = torch.tanh(torch.nn.functional.linear(h, p["contact_ae.contact_enc_mlp.2.weight"],
                                               p["contact_ae.contact_enc_mlp.2.bias"]))
    lat = ec if only_contact else torch.cat([mlp("env_mlp", len(priv_units), priv), ec], -1)
    x = torch.cat([obs, lat], -1)
    a = mlp("actor_mlp", len(units), x)
    mu = torch.nn.functional.linear(a, p["mu.weight"], p["mu.bias"])
    c = mlp("critic_mlp", len(units), x)
    values = torch.nn.functional.linear(c, p["value.weight"], p["value.bias"])
    logstd = mu * 0 + p["sigma"]
    sigma = torch.exp(logstd)
    nlp = ot.gaussian_neglogp(d["actions"][idx].double(), mu, sigma, logstd)
    entropy = (0.5 + ot.LOG_SQRT_2PI + logstd).sum(-1)
    hp = orc.hp
    adv, old_nlp = d["advantages"][idx].double(), d["neglogpacs"][idx].double()
    vp, ret = d["values"][idx].double(), d["returns"][idx].double()
    ratio = torch.exp(old_nlp - nlp)
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - hp["e_clip"], 1 + hp["e_clip"]))
    vc = vp + (values - vp).clamp(-hp["e_clip"], hp["e_clip"])
    c_loss = torch.max((values - ret) ** 2, (vc - ret) ** 2)
    b_loss = (torch.clamp_max(-mu + 1.1, 0.0) ** 2 + torch.clamp_max(mu - 1.1, 0.0) ** 2).sum(-1)
    loss = a_loss.mean() + 0.5 * c_loss.mean() * hp["critic_coef"] - entropy.mean() * hp["entropy_coef"] \
        + b_loss.mean() * hp["bounds_loss_coef"]
    loss.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}


@pytest.mark.parametrize("case", ["contacts_small", "only_contact_small", "contacts_full"])
def test_teacher_contact_step_gradient_vs_float64(case):
    if case == "contacts_full":
        N, T, Ep, units, priv_units, P, E, oc = 4096, 32, 8, [512, 256, 128], [256, 128, 8], 400, 8, False
    else:
        N, T, Ep, units, priv_units, P, E = 64, 8, 2, [64, 32, 16], [32, 16, 8], 37, 8
        oc = case.startswith("only")
    init, ro, perm = _problem(N, T, units, priv_units, P, E, oc)
    eng = _engine(N, T, Ep, units, priv_units, P, E, oc, init, perm)
    eng.prepare(_ro_cuda(ro))
    eng.fwd_bwd(0, 0)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in eng.param_views(eng.grads).items()}
    ref = _step0_grad64(init, ro, perm, N, T, Ep, units, priv_units, oc)
    flat_ref = torch.cat([ref[k].reshape(-1) for k in got]).numpy()
    flat_got = torch.cat([got[k].reshape(-1) for k in got]).numpy()
    np.testing.assert_allclose(flat_got, flat_ref, atol=2e-4 * np.abs(flat_ref).max(), rtol=2e-3)
    for k in got:    # the encoder's own gradient is exercised, the decoder's slots stay zero
        if k.startswith("contact_ae.contact_dec_mlp") or (oc and k.startswith("env_mlp")):
            assert not got[k].any(), k
        elif k.startswith("contact_ae.contact_enc_mlp") and k.endswith("weight"):
            assert got[k].abs().max() > 0, k
            np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), atol=2e-4 * ref[k].abs().max().item(), rtol=2e-3)


@pytest.mark.parametrize("oc", [False, True])
def test_teacher_contact_update_reproducible_and_frozen_params(oc):
    N, T, Ep, units, priv_units, P, E = 256, 16, 4, [64, 32, 16], [32, 16, 8], 37, 8
    init, ro, perm = _problem(N, T, units, priv_units, P, E, oc, seed=99)
    out = []
    for _ in range(2):
        eng = _engine(N, T, Ep, units, priv_units, P, E, oc, init, perm)
        eng.prepare(_ro_cuda(ro))
        eng.update()
        eng.prepare(_ro_cuda(ro))
        eng.update()
        torch.cuda.synchronize()
        out.append(eng)
    a, b = out
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    va, ma, vv = a.param_views(), a.param_views(a.adam_m), a.param_views(a.adam_v)
    for k in va:
        frozen = k.startswith("contact_ae.contact_dec_mlp") or (oc and k.startswith("env_mlp"))
        if frozen:
            assert torch.equal(va[k].cpu(), init[k]), k
            assert not ma[k].any() and not vv[k].any(), k
        else:
            assert not torch.equal(va[k].cpu(), init[k]), k
    assert torch.isfinite(a.stats).all()


def test_teacher_contact_inference_and_model():
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    torch.manual_seed(3)
    m = ActorCriticSplit(dict(actor_units=[64, 32, 16], actions_num=6, input_shape=(15,), priv_mlp_units=[32, 16, 8],
                              priv_info_dim=64, priv_info=True, gt_contacts_info=True, only_contact=False,
                              contacts_mlp_units=[8], num_contact_points=37)).cuda()
    rows = 1000
    g = torch.Generator().manual_seed(5)
    obs, priv = torch.randn(rows, 15, generator=g), torch.randn(rows, 64, generator=g)
    contacts = (torch.rand(rows, 37, generator=g) < 0.3).float()
    mu, latent = m.act_inference(dict(obs=obs.cuda(), priv_info=priv.cuda(), contacts=contacts.cuda()))
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}

    def mlp(prefix, n, x):
        for i in range(n):
            x = torch.tanh(x @ sd[f"{prefix}.mlp.{2 * i}.weight"].T + sd[f"{prefix}.mlp.{2 * i}.bias"])
        return x
    ec, _ = _enc64(contacts.double(), sd["contact_ae.contact_enc_mlp.0.weight"], sd["contact_ae.contact_enc_mlp.0.bias"],
                   sd["contact_ae.contact_enc_mlp.2.weight"], sd["contact_ae.contact_enc_mlp.2.bias"])
    lat = torch.cat([mlp("env_mlp", 3, priv.double()), ec], -1)
    x = torch.cat([obs.double(), lat], -1)
    mu_ref = mlp("actor_mlp", 3, x) @ sd["mu.weight"].T + sd["mu.bias"]
    assert latent.shape == (rows, 16)
    np.testing.assert_allclose(latent.cpu().numpy(), lat.numpy(), atol=1e-5)
    np.testing.assert_allclose(mu.cpu().numpy(), mu_ref.numpy(), atol=1e-5)
    enc = m.contact_ae.forward_enc(contacts.cuda())
    np.testing.assert_allclose(enc.cpu().numpy(), ec.numpy(), atol=2e-6)


def test_opcheck_contact_ops():
    import isaacgyminsertion_amd.ops  # noqa: F401
    o = torch.ops.mi355ppo
    tests = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
    g = torch.Generator(device="cuda").manual_seed(0)
    C = (torch.rand(50, 37, device="cuda", generator=g) < 0.3).float()
    params = 0.1 * torch.randn(32 * 37 + 32 + 8 * 32 + 8, device="cuda", generator=g)
    torch.library.opcheck(o.contact_encoder_fwd, (C, params, 8), test_utils=tests)
    _, hid = o.contact_encoder_fwd(C, params, 8)
    torch.library.opcheck(o.contact_encoder_bwd, (C, params, hid, torch.randn(50, 8, device="cuda", generator=g)),
                          test_utils=tests)
    N, T, Ep, units, priv_units, P, E = 64, 8, 2, [64, 32, 16], [32, 16, 8], 37, 8
    init, ro, perm = _problem(N, T, units, priv_units, P, E, False)
    eng = _engine(N, T, Ep, units, priv_units, P, E, False, init, perm)
    eng.set_rollout(_ro_cuda(ro))
    ic, fc = eng._cfg_args()
    torch.library.opcheck(o.ppo_minibatch_fwd_bwd, (eng._ro, eng.state_list(), ic, fc, 0, 0, -1), test_utils=tests)
    obs, priv = torch.randn(10, 15, device="cuda"), torch.randn(10, 64, device="cuda")
    cts = (torch.rand(10, P, device="cuda") < 0.3).float()
    torch.library.opcheck(o.actor_critic_infer_contacts, (eng.state_list(), ic, fc, obs, priv, cts, False, True),
                          test_utils=tests)
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    torch.library.opcheck(o.rollout_policy_step_contacts,
                          (eng.state_list(), ic, fc, obs, priv, cts, False, torch.randn(10, 6, device="cuda"), None,
                           None, None, z(10, P), z(10, 6), z(10), z(10, 1), z(10, 6), z(10, 6), z(10, 6), z(10, 1)),
                          test_utils=tests)
