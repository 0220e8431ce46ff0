"""The teacher step OFF its default widths, with and without ground-truth contacts, against the CPU oracle
(oracle/teacher.py, pinned to the reference's goldens with and without contacts): a whole update per shape, and
inference / the rollout policy step on the same engines against float64.

Every other GPU test of the teacher has priv_units[-1] == 8 (the fused latent backward, k_latent_bwd) and
obs + latent (+ embedding) <= 32 (one 32-wide k-tile of the padded first trunk layer).  The cases here are chosen by the
branch of make_plan / teacher_fwd_bwd they reach; where that branch is a launch the profiler can see, its class is asserted
(the launch counts in the case tables below), so a case cannot silently start testing something else.

Tolerances are test_ragged_configs_match_oracle's (tests/test_gpu_edges.py), unchanged: returns_raw bit-equal, advantages
5e-5, step-0 flat gradient 2e-4 of the largest entry + 2e-3 relative, the four loss columns of every optimizer step
2e-4 relative + 2e-6, final parameters steps * lr * 0.05, scattered mus 2e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRIV, ACT = 64, 6
DEFAULT_UNITS, DEFAULT_PRIV_UNITS = [512, 256, 128], [256, 128, 8]
FOUR_UNITS, FOUR_PRIV_UNITS = [96, 64, 48, 32], [48, 32, 16, 8]

# profiler classes (csrc/prof.h) a case may pin.  "other" counts k_latent_dgrad, k_contact_fwd and k_contact_bwd in a
# training step (the only PC_OTHER launches of teacher_fwd_bwd).  K_LATG: the generic latent data gradient
# (dZ1 . W1p, EPI_TANHGRAD over all xld columns) is a product with a k-contiguous A and a row-major B launched on its own.
# The only other products of that form are env_mlp's data gradients, and in every case here those contract over fewer than 32
# columns (the generic kernel) or ride in a level launch -- so that instantiation of the tile kernel running once IS the
# branch (every case has 2 * u0 a multiple of 32, which the tile kernel needs).
K_LATG = "gemm_dma_kernel<64,true,false>"
K_LATB, K_HEAD, K_GENERIC, K_OTHER, K_FWD12 = "k_latent_bwd", "gemm_dma_head_kernel<true>", "gemm_f32_kernel<*>", "other", "k_fwd12"
K_RB_TRUNK, K_RB_ENV, K_TRUNK_LOSS, K_LOSS = "k_rb_level#trunk3", "k_rb_level#env2", "k_trunk_loss", "k_loss"


def _problem(N, T, units, priv_units, obs_dim=15, P=0, E=0, only_contact=False, seed=1234, done_p=0.05):
    """synth.teacher_problem, plus -- with contacts -- random 0/1 contacts, random encoder / decoder / first-trunk-layer
    parameters, and the rollout's old mus / values / neglogpacs recomputed with THAT network (the synthetic rollout's
    contract: the old policy is the initial network, so PPO ratios start at 1, away from the clipped loss's kinks)."""
    from oracle import synth, teacher as ot
    base, ro, perm = synth.teacher_problem(N, T, units, priv_units, obs_dim=obs_dim, seed=seed, done_p=done_p)
    if not P:
        return base, ro, perm
    g = torch.Generator().manual_seed(seed + 1)
    init = type(base)()
    for k, shp in ot.teacher_param_shapes(obs_dim, PRIV, ACT, units, priv_units, P, E, only_contact).items():
        if k in base and tuple(base[k].shape) == tuple(shp):
            init[k] = base[k].clone().float()
        elif len(shp) == 2:
            init[k] = torch.randn(*shp, generator=g) / np.sqrt(shp[1])
        else:
            init[k] = 0.05 * torch.randn(*shp, generator=g)
    ro = dict(ro)
    ro["contacts"] = (torch.rand(T, N, P, generator=g) < 0.15).float()
    rs_o, rs_p, rs_v = ot.RmsState(obs_dim), ot.RmsState(PRIV), ot.RmsState(1)
    with torch.no_grad():
        mu, logstd, value, _ = ot.actor_critic(init, rs_o.normalize(ro["obses"].reshape(-1, obs_dim)),
                                               rs_p.normalize(ro["priv_info"].reshape(-1, PRIV)), len(priv_units),
                                               len(units), ro["contacts"].reshape(-1, P), only_contact)
        sigma = torch.exp(logstd)
        eps = (ro["actions"] - ro["mus"]) / ro["sigmas"]          # the rollout's own exploration noise
        ro["mus"], ro["sigmas"] = mu.reshape(T, N, ACT).contiguous(), sigma.reshape(T, N, ACT).contiguous()
        ro["actions"] = (ro["mus"] + ro["sigmas"] * eps).contiguous()
        ro["values"] = rs_v.unnormalize(value).reshape(T, N, 1).contiguous()
        ro["neglogpacs"] = ot.gaussian_neglogp(ro["actions"], ro["mus"], ro["sigmas"], torch.log(ro["sigmas"])).contiguous()
    return init, ro, perm


def _engine(N, T, Ep, units, priv_units, init, perm, obs_dim=15, P=0, E=0, only_contact=False, **kw):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    eng = TeacherEngine(N, T, Ep, units=units, priv_units=priv_units, perm=perm, obs_dim=obs_dim, contact_points=P,
                        contact_emb=E, only_contact=only_contact, **kw)
    eng.load_params(init)
    return eng


def _frozen(k, only_contact):
    return k.startswith("contact_ae.contact_dec_mlp") or (only_contact and k.startswith("env_mlp"))


def _update_vs_oracle(N, T, Ep, units, priv_units, obs_dim=15, P=0, E=0, only_contact=False, max_steps=None,
                      kernels=None, absent=(), seed=1234):
    """prepare, the step-0 gradient, then EVERY optimizer step of one update (or max_steps of them) with fwd_bwd + apply."""
    from isaacgyminsertion_amd import _lib
    from oracle import teacher as ot
    init, ro, perm = _problem(N, T, units, priv_units, obs_dim, P, E, only_contact, seed=seed)
    eng = _engine(N, T, Ep, units, priv_units, init, perm, obs_dim, P, E, only_contact)
    orc = ot.TeacherOracle(init, perm, N, T, Ep, units, priv_units, obs_dim=obs_dim, contact_points=P, contact_emb=E,
                           only_contact=only_contact)
    d = orc.prepare(ro)
    eng.prepare(ro)
    torch.cuda.synchronize()
    assert torch.equal(eng.returns_raw.cpu(), orc.returns_raw)
    np.testing.assert_allclose(eng.env_major(eng.advantages).cpu().numpy(), d["advantages"].numpy(), atol=5e-5)
    st = orc.update(record_grads=1, max_steps=max_steps)
    _lib.prof_enable(True)
    try:
        eng.fwd_bwd(0, 0)
        torch.cuda.synchronize()
        classes = {}
        for c in _lib.prof_read():
            name = c["name"].split(":")[0]
            classes[name] = classes.get(name, 0) + c["launches"]
    finally:
        _lib.prof_enable(False)
    print("launches of step 0:", {k: v for k, v in sorted(classes.items()) if v})
    for name, count in (kernels or {}).items():
        assert classes.get(name, 0) == count, (name, count, classes)
    for name in absent:
        assert not any(k.startswith(name) and v for k, v in classes.items()), (name, classes)
    # ---- step-0 gradient of every parameter
    ref = st["grads"][0].numpy()
    got = eng.packed(eng.grads).cpu().numpy()
    gmax = np.abs(ref).max()
    print(f"step-0 gradient: max |diff| / max |ref| = {np.abs(got - ref).max() / gmax:.3e}")
    np.testing.assert_allclose(got, ref, atol=2e-4 * gmax, rtol=2e-3)
    if P:
        off = 0
        gv = {k: v.cpu() for k, v in eng.param_views(eng.grads).items()}
        for k, v in init.items():
            r = ref[off:off + v.numel()].reshape(v.shape)
            off += v.numel()
            if _frozen(k, only_contact):          # grad None in the reference
                assert not gv[k].any() and not r.any(), k
            elif k.startswith("contact_ae.contact_enc_mlp") and k.endswith("weight"):   # the encoder on its own scale
                assert gv[k].abs().max() > 0 and np.abs(r).max() > 0, k
                np.testing.assert_allclose(gv[k].numpy(), r, atol=2e-4 * np.abs(r).max(), rtol=2e-3, err_msg=k)
    # ---- the rest of the update
    eng.apply(0)
    slot = 1
    total = Ep * eng.n_mb if max_steps is None else max_steps
    for e in range(Ep):
        for i in range(eng.n_mb):
            if (e == 0 and i == 0) or slot >= total:
                continue
            eng.fwd_bwd(i, slot)
            eng.apply(slot)
            slot += 1
    torch.cuda.synchronize()
    assert slot == total == len(st["a_losses"])
    s = eng.stats.cpu().numpy()
    for j, nm in enumerate(["a_losses", "c_losses", "b_losses", "entropies"]):
        np.testing.assert_allclose(s[:slot, j], np.array([x.item() for x in st[nm]]), rtol=2e-4, atol=2e-6, err_msg=nm)
    pd = np.abs(eng.packed().cpu().numpy() - orc.flat_params().numpy()).max()
    print(f"final parameters after {slot} steps: max |diff| = {pd:.3e} (bound {slot * 2.5e-4 * 0.05:.3e})")
    np.testing.assert_allclose(eng.packed().cpu().numpy(), orc.flat_params().numpy(), atol=slot * 2.5e-4 * 0.05)
    # update_mu_sigma: the scattered policy means (of the rows the steps that ran have visited)
    rows = perm[:eng.mb * min(slot, eng.n_mb)].numpy() if max_steps is not None else slice(None)
    np.testing.assert_allclose(eng.env_major(eng.mus_w).cpu().numpy()[rows], orc.data["mus"].detach().numpy()[rows],
                               atol=2e-5)
    if P:   # frozen tensors and their Adam moments bit-unchanged; everything else moved
        va, ma, vv = eng.param_views(), eng.param_views(eng.adam_m), eng.param_views(eng.adam_v)
        for k in va:
            if _frozen(k, only_contact):
                assert torch.equal(va[k].cpu(), init[k]), k
                assert not ma[k].any() and not vv[k].any(), k
            else:
                assert not torch.equal(va[k].cpu(), init[k]), k
    return eng


# N, T, mini_epochs: mb = 200 = one whole 128-row tile and a partial one; 9 optimizer steps
SMALL = (100, 6, 3)

NO_CONTACT_CASES = {
    # name: (N, T, Ep), units, priv_units, obs_dim, max_steps, {class: launches in step 0}, (classes that must not run)
    # generic latent data gradient (EPI_TANHGRAD GEMM over the xld columns); the 5-wide latent layer as a launch of its own
    # because the layer before it has a 24-wide input (the head kernel needs whole 32-wide k-tiles)
    "latent5": (SMALL, [48, 40, 24], [24, 16, 5], 15, None, {K_LATB: 0, K_OTHER: 0, K_LATG: 1, K_HEAD: 0}, ()),
    # the same latent width riding in the epilogue of the layer before it (gemm_with_head, head_n = 5)
    "latent5_head": (SMALL, [48, 40, 24], [32, 16, 5], 15, None, {K_LATB: 0, K_OTHER: 0, K_LATG: 1, K_HEAD: 1}, ()),
    # latent > 8: plain last env layer, generic latent data gradient, xw = 27
    "latent12": (SMALL, [48, 40, 24], [32, 16, 12], 15, None, {K_LATB: 0, K_OTHER: 0, K_LATG: 1, K_HEAD: 0}, ()),
    # xw = 39 -> xld = 64: a second k-tile of the padded first trunk layer, two-layer env_mlp
    "latent24": (SMALL, [48, 40, 24], [32, 24], 15, None, {K_LATB: 0, K_OTHER: 0, K_LATG: 1, K_HEAD: 0}, ()),
    # the fused latent backward (k_latent_bwd) with xld = 64 (xw = 48)
    "wide_obs": (SMALL, [48, 40, 24], [24, 16, 8], 40, None, {K_LATB: 1, K_OTHER: 0, K_LATG: 0}, ()),
    # the default network behind a 48-wide input, mb = 2048, optimizer step 0 only: the row-block levels run (the env level
    # with k_latent_bwd's work at the head of its blocks, so that kernel does not launch); the fused env_mlp + first-trunk-layer
    # forward (k_fwd12) and the first-layer weight gradient from the dZ1 tiles both decline xld = 64: that weight gradient
    # rides with the first env layer's ("#env1+")
    "wide_obs_default_net": ((256, 16, 2), DEFAULT_UNITS, DEFAULT_PRIV_UNITS, 40, 1,
                             {K_LATB: 0, K_OTHER: 0, K_LATG: 0, K_RB_TRUNK: 1, K_RB_ENV: 1, K_TRUNK_LOSS: 1, K_HEAD: 1,
                              "gemm_dma_wgrad_multi_kernel#env1+": 1}, (K_FWD12,)),
    # xw = 64: no free padding column in the second k-tile (mb = 256 and widths of whole tiles: the tile kernels run the
    # first layer's products);  xw = 65: a third k-tile (xld = 96), at ragged widths (the generic kernel) and at whole tiles
    "xw64": ((64, 8, 2), [128, 64, 32], [32, 16, 8], 56, None, {K_LATB: 1, K_OTHER: 0, K_LATG: 0}, ()),
    "xw65": (SMALL, [48, 40, 24], [24, 16, 8], 57, None, {K_LATB: 1, K_OTHER: 0, K_LATG: 0}, ()),
    "xw65_whole_tiles": ((64, 8, 2), [128, 64, 32], [32, 16, 8], 57, None, {K_LATB: 1, K_OTHER: 0, K_LATG: 0}, ()),
    # one env layer (no second-to-last layer for k_latent_bwd): k_latent_dgrad<1, 8> (2 * u0 = 256), <4, 8> (1024), and
    # the generic GEMM when 2 * u0 is not a multiple of 256
    "one_env_layer_u128": (SMALL, [128, 64, 32], [8], 15, None, {K_LATB: 0, K_OTHER: 1, K_LATG: 0}, ()),
    "one_env_layer_u512": (SMALL, [512, 64, 32], [8], 15, None, {K_LATB: 0, K_OTHER: 1, K_LATG: 0}, ()),
    "one_env_layer_u96": (SMALL, [96, 64, 32], [8], 15, None, {K_LATB: 0, K_OTHER: 0, K_LATG: 1}, ()),
    # second-to-last env layer wider than k_latent_bwd's 256: k_latent_dgrad<1, 8>
    "wide_second_to_last": (SMALL, [128, 64, 32], [320, 8], 15, None, {K_LATB: 0, K_OTHER: 1, K_LATG: 0, K_HEAD: 0}, ()),
    # one trunk layer: layer 0 is also the last layer (the loss kernel writes the interleaved dZ of layer 0)
    "one_trunk_layer_64": (SMALL, [64], [24, 16, 8], 15, None, {K_LATB: 1, K_TRUNK_LOSS: 0, K_LOSS: 1}, ()),
    "one_trunk_layer_128": (SMALL, [128], [24, 16, 8], 15, None, {K_LATB: 1, K_TRUNK_LOSS: 0, K_LOSS: 1}, ()),
    # four layers per MLP: 4 + 1 + 8 + 16 = 29 gradient segments
    "four_layers": (SMALL, FOUR_UNITS, FOUR_PRIV_UNITS, 15, None, {K_LATB: 1, K_OTHER: 0, K_LATG: 0}, ()),
}


@pytest.mark.parametrize("case", list(NO_CONTACT_CASES))
def test_update_off_the_default_widths_matches_oracle(case):
    (N, T, Ep), units, priv_units, obs_dim, max_steps, kernels, absent = NO_CONTACT_CASES[case]
    _update_vs_oracle(N, T, Ep, units, priv_units, obs_dim=obs_dim, max_steps=max_steps, kernels=kernels, absent=absent)


CT_UNITS, CT_PRIV_UNITS = [64, 32, 16], [32, 16, 8]
# k_contact_fwd + k_contact_bwd once each; contacts switch the fused latent backward and k_latent_dgrad off: the generic one
CT = {K_LATB: 0, K_OTHER: 2, K_LATG: 1}

CONTACT_CASES = {
    # name: (N, T, Ep), units, priv_units, P, E, only_contact, max_steps, {class: launches}
    # embedding widths: xw = 24, 32 (column 31 live: no free padding column), 39 and 55 (xld = 64); the e < E guards
    "E1": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 37, 1, False, None, CT),
    "E9": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 37, 9, False, None, CT),
    "E16": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 37, 16, False, None, CT),
    "E32": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 37, 32, False, None, CT),
    # ragged rows: mb = 37 (one 32-row forward wave and 5 rows of the next, a partial 128-row backward block) and mb = 300
    # (two whole backward blocks and 44 rows); T > 1, so minibatch rows are permuted rows of the (T, N, P) arena
    "rows37": ((37, 5, 5), CT_UNITS, CT_PRIV_UNITS, 37, 5, False, None, CT),
    "rows300": ((100, 6, 2), CT_UNITS, CT_PRIV_UNITS, 37, 8, False, None, CT),
    # contact points: fewer than one half-chunk of 16, the scalar loader with a one-column tail, the float4 loader with
    # a 4-column last chunk
    "P5": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 5, 8, False, None, CT),
    "P33": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 33, 8, False, None, CT),
    "P36": ((64, 8, 2), CT_UNITS, CT_PRIV_UNITS, 36, 8, False, None, CT),
    # only_contact: the embedding sits at column obs, env_mlp is neither run nor trained
    "only_contact_E4": ((64, 8, 2), CT_UNITS, [32, 16, 4], 37, 4, True, None, CT),
    "only_contact_E16": ((64, 8, 2), CT_UNITS, [32, 16, 16], 37, 16, True, None, CT),
    # four layers per MLP with contacts: 4 + 1 + 8 + 4 + 16 = 33 gradient segments, the most make_plan accepts
    "four_layers": (SMALL, FOUR_UNITS, FOUR_PRIV_UNITS, 37, 8, False, None, CT),
    # the default network with the reference's 400 contact points, mb = 2048, optimizer step 0 only
    "default_net": ((256, 16, 2), DEFAULT_UNITS, DEFAULT_PRIV_UNITS, 400, 8, False, 1,
                    dict(CT, **{K_RB_TRUNK: 1, K_RB_ENV: 1, K_TRUNK_LOSS: 1, K_HEAD: 1, K_FWD12: 0})),
}


@pytest.mark.parametrize("case", list(CONTACT_CASES))
def test_contact_update_off_the_default_widths_matches_oracle(case):
    (N, T, Ep), units, priv_units, P, E, oc, max_steps, kernels = CONTACT_CASES[case]
    _update_vs_oracle(N, T, Ep, units, priv_units, P=P, E=E, only_contact=oc, max_steps=max_steps, kernels=kernels)


# ---- inference and the rollout policy step on the same engines ---------------------------------------------------
INFER_CASES = {
    # name: units, priv_units, obs_dim, P, E, only_contact          (engine 64 x 8 / 2: chunks of mb = 256 rows)
    "latent12": ([48, 40, 24], [32, 16, 12], 15, 0, 0, False),
    "wide_obs": ([48, 40, 24], [24, 16, 8], 40, 0, 0, False),          # xld = 64: k_pad_w1 fills two k-tiles
    "xw65": ([48, 40, 24], [24, 16, 8], 57, 0, 0, False),              # xld = 96
    "contacts_E9": (CT_UNITS, CT_PRIV_UNITS, 15, 37, 9, False),        # xw = 32: column 31 live
    "contacts_E16": (CT_UNITS, CT_PRIV_UNITS, 15, 37, 16, False),      # xld = 64
    "only_contact_E4": (CT_UNITS, [32, 16, 4], 15, 37, 4, True),
}
ROWS = 2 * 256 + 77      # larger than mb = 256 (the chunk loop), neither a multiple of 32 nor of mb


def _infer_setup(case, rows=ROWS, **engine_kw):
    units, priv_units, obs_dim, P, E, oc = INFER_CASES[case]
    N, T, Ep = 64, 8, 2
    init, ro, perm = _problem(N, T, units, priv_units, obs_dim, P, E, oc, seed=77)
    g = torch.Generator().manual_seed(1000 + len(case))
    init["sigma"] = 0.3 * torch.randn(ACT, generator=g)
    eng = _engine(N, T, Ep, units, priv_units, init, perm, obs_dim, P, E, oc, **engine_kw)
    assert ROWS > eng.mb and ROWS % eng.mb and ROWS % 32
    # running statistics away from their initial (0, 1, 1)
    mean_o, var_o = 0.3 * torch.randn(obs_dim, generator=g).double(), (0.5 + torch.rand(obs_dim, generator=g)).double()
    mean_p, var_p = 0.3 * torch.randn(PRIV, generator=g).double(), (0.5 + torch.rand(PRIV, generator=g)).double()
    eng.rms_obs[:obs_dim], eng.rms_obs[obs_dim:2 * obs_dim] = mean_o.cuda(), var_o.cuda()
    eng.rms_priv[:PRIV], eng.rms_priv[PRIV:2 * PRIV] = mean_p.cuda(), var_p.cuda()
    obs = 1.5 * torch.randn(rows, obs_dim, generator=g) + 0.2
    priv = torch.randn(rows, PRIV, generator=g)
    contacts = (torch.rand(rows, P, generator=g) < 0.2).float() if P else None
    noise = torch.randn(rows, ACT, generator=g)
    p64 = {k: v.double() for k, v in init.items()}

    def norm64(x, mean, var):     # running_mean_std.py:91-92
        return torch.clamp((x.double() - mean) / torch.sqrt(var + 1e-5), -5.0, 5.0)

    def ref(normalize):
        from oracle import teacher as ot
        o = norm64(obs, mean_o, var_o) if normalize else obs.double()
        q = norm64(priv, mean_p, var_p) if normalize else priv.double()
        with torch.no_grad():
            return ot.actor_critic(p64, o, q, len(priv_units), len(units), contacts.double() if P else None, oc)
    return eng, obs, priv, contacts, noise, ref, (obs_dim, P, E, oc, priv_units)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", list(INFER_CASES))
def test_infer_off_the_default_widths_matches_float64(case, normalize):
    """infer / infer_contacts (mu, normalised value, latent_gt) against the oracle's actor_critic in float64 at
    test_infer_matches_oracle's bounds."""
    eng, obs, priv, contacts, _, ref, (obs_dim, P, E, oc, priv_units) = _infer_setup(case)
    if P:
        mu, val, lat = eng.infer_contacts(obs, priv, contacts, want_latent=True, normalize=normalize)
    else:
        mu, val, lat = eng.infer(obs, priv, want_latent=True, normalize=normalize)
    torch.cuda.synchronize()
    m, _, v, e = ref(normalize)
    assert lat.shape == (ROWS, E if oc else priv_units[-1] + E)
    np.testing.assert_allclose(mu.cpu().numpy(), m.numpy(), atol=2e-6, rtol=1e-4)
    np.testing.assert_allclose(val.cpu().numpy(), v.numpy(), atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(lat.cpu().numpy(), e.numpy(), atol=2e-6, rtol=1e-4)


def test_infer_contacts_under_the_adaptive_schedule_matches_float64():
    """The schedule's extra int behind the contact fields must not change what the latent is: the same engine as
    contacts_E16 built with lr_schedule="adaptive", 33 rows (one full 32-row block and a ragged row), the bounds above."""
    eng, obs, priv, contacts, _, ref, (_, P, E, oc, priv_units) = _infer_setup("contacts_E16", rows=33, lr_schedule="adaptive")
    assert eng.cfg.lr_schedule == 1 and P and not oc
    mu, val, lat = eng.infer_contacts(obs, priv, contacts, want_latent=True, normalize=True)
    torch.cuda.synchronize()
    m, _, v, e = ref(True)
    assert lat.shape == (33, priv_units[-1] + E)
    np.testing.assert_allclose(mu.cpu().numpy(), m.numpy(), atol=2e-6, rtol=1e-4)
    np.testing.assert_allclose(val.cpu().numpy(), v.numpy(), atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(lat.cpu().numpy(), e.numpy(), atol=2e-6, rtol=1e-4)


@pytest.mark.parametrize("case", list(INFER_CASES))
def test_rollout_policy_step_off_the_default_widths_matches_float64(case):
    """rollout_policy_step / rollout_policy_step_contacts on given noise against a float64 restatement of model_act +
    the storage writes of play_steps (frozen_ppo.py:343-366, 655-665), at the bounds tests/test_gpu_rollout.py holds the same
    quantities to against the reference (mus / actions / values 2e-5, sigmas 1e-6, neglogp 5e-5, 1e-5 relative); the arena
    slot holds the raw observations, privileged inputs and contacts bit for bit."""
    from oracle import teacher as ot
    eng, obs, priv, contacts, noise, ref, (obs_dim, P, E, oc, priv_units) = _infer_setup(case)
    f = dict(dtype=torch.float32, device="cuda:0")
    n = ROWS
    o = dict(obses=torch.zeros(n, obs_dim, **f), priv=torch.zeros(n, PRIV, **f), actions=torch.zeros(n, ACT, **f),
             nlp=torch.zeros(n, **f), values=torch.zeros(n, 1, **f), mus=torch.zeros(n, ACT, **f),
             sigmas=torch.zeros(n, ACT, **f), clamped=torch.zeros(n, ACT, **f), vout=torch.zeros(n, 1, **f))
    rms_v = torch.tensor([0.5, 4.0, 100.0], dtype=torch.float64, device="cuda:0")
    d_obs, d_priv, d_noise = obs.cuda(), priv.cuda(), noise.cuda()
    if P:
        d_ct, ct_t = contacts.cuda(), torch.zeros(n, P, **f)
        torch.ops.mi355ppo.rollout_policy_step_contacts(eng.state_list(), *eng._cfg_args(), d_obs, d_priv, d_ct, True,
                                                        d_noise, rms_v, o["obses"], o["priv"], ct_t, o["actions"], o["nlp"],
                                                        o["values"], o["mus"], o["sigmas"], o["clamped"], o["vout"])
    else:
        torch.ops.mi355ppo.rollout_policy_step(eng.state_list(), *eng._cfg_args(), d_obs, d_priv, True, d_noise, rms_v,
                                               o["obses"], o["priv"], o["actions"], o["nlp"], o["values"], o["mus"],
                                               o["sigmas"], o["clamped"], o["vout"])
    torch.cuda.synchronize()
    mu, logstd, value, _ = ref(True)
    sigma = torch.exp(logstd)
    action = mu + sigma * noise.double()                                        # Normal(mu, sigma).sample() on this noise
    nlp = ot.gaussian_neglogp(action, mu, sigma, logstd)
    value = np.sqrt(4.0 + 1e-5) * torch.clamp(value, -5.0, 5.0) + 0.5           # value_mean_std(values, unnorm=True)
    assert torch.equal(o["obses"].cpu(), obs) and torch.equal(o["priv"].cpu(), priv)
    if P:
        assert torch.equal(ct_t.cpu(), contacts)
    for k, want, atol in (("mus", mu, 2e-5), ("sigmas", sigma, 1e-6), ("actions", action, 2e-5),
                          ("clamped", action.clamp(-1.0, 1.0), 2e-5), ("values", value, 2e-5), ("vout", value, 2e-5),
                          ("nlp", nlp, 5e-5)):
        np.testing.assert_allclose(o[k].cpu().numpy(), want.numpy(), atol=atol, rtol=1e-5, err_msg=k)
    assert float(action.abs().max()) > 1.0        # the clamp is exercised
