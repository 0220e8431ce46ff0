"""The latent student's loss with its latent term live (offline_train.train.latent_loss; ext_adapt.py:827 without the
comment sign) on the device: ``distill_loss_value_grad`` (csrc/rollout.h k_distill_loss) against float64 autograd and
against ``bc_loss_fwd_bwd``, and ``ExtrinsicAdapt`` on the buffer and weights of tests/golden/student_latent.npz -- what
the reference's own modules gave for minibatch 0 at (action_scale, latent_scale) = (1, 0), (1, 1), (1.3, 0.7)
(tests/golden/make_golden_student_latent.py).

Tolerances: the op's losses 1e-6 relative (fp64 sums on both sides), its gradients 1e-6 of the largest entry + 1e-5
relative (elementwise fp32); the trainer's losses 2e-4 relative and its raw step-0 gradients by
test_student_update_matches_reference's rule (tests/test_gpu_student.py): max(1e-3 of the tensor's largest entry, 1e-6 of
the largest overall, 4 x the reference's own fp32 noise) + 1e-3 relative."""
import numpy as np
import pytest
import torch

from tests import latent_student_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = [1.0, 1.0, 0.1, 1.0, 1.0, 1.0]


def _inputs(rows, L, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand(rows, 6, generator=g) * 2.8 - 1.4          # entries beyond +-1 ...
    act = torch.rand(rows, 6, generator=g) * 2.8 - 1.4
    flat = mu.view(-1)
    flat[0::7] = 1.0                                            # ... and exactly on the clamp's corners
    flat[3::11] = -1.0
    assert bool((mu.abs() > 1).any()) or rows == 1
    return mu, act, torch.randn(rows, L, generator=g), torch.randn(rows, L, generator=g)


@pytest.mark.parametrize("rows", [1, 16, 37, 70])
@pytest.mark.parametrize("L", [8, 5])
def test_distill_loss_matches_float64_autograd(rows, L):
    from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
    mu, act, lat, lgt = _inputs(rows, L, 100 * rows + L)
    a_s, l_s = 1.3, 0.7
    w = torch.tensor(WEIGHTS)
    m64, l64 = mu.double().requires_grad_(True), lat.double().requires_grad_(True)
    la64 = (((torch.clamp(m64, -1, 1) - torch.clamp(act.double(), -1, 1)) ** 2) * w.double()).sum()
    ll64 = torch.nn.MSELoss()(l64, lgt.double())
    (a_s * la64 + l_s * ll64).backward()
    args = [t.to(DEV) for t in (mu, act, w, lat, lgt)]
    la, ll, dmu, dlat = torch.ops.mi355ppo.distill_loss_value_grad(*args, a_s, l_s)
    assert la.shape == () and ll.shape == () and dmu.shape == mu.shape and dlat.shape == lat.shape
    np.testing.assert_allclose(la.item(), la64.item(), rtol=1e-6)
    np.testing.assert_allclose(ll.item(), ll64.item(), rtol=1e-6)
    for got, ref, nm in ((dmu, m64.grad, "dmu"), (dlat, l64.grad, "dlatent")):
        r = ref.numpy()
        np.testing.assert_allclose(got.cpu().numpy(), r, atol=1e-6 * np.abs(r).max(), rtol=1e-5, err_msg=nm)
    # the action term is bc_loss_fwd_bwd's: same value, its gradient times action_scale; no latent gradient at scale 0
    la0, _, dmu0, dlat0 = torch.ops.mi355ppo.distill_loss_value_grad(*args, a_s, 0.0)
    bc, dbc = torch.ops.mi355ppo.bc_loss_fwd_bwd(args[0], args[1], args[2], True)
    np.testing.assert_allclose(la0.item(), bc.item(), rtol=1e-6)
    np.testing.assert_allclose(dmu0.cpu().numpy(), (dbc * a_s).cpu().numpy(), rtol=1e-6, atol=0)
    assert float(dlat0.abs().max()) == 0.0
    # fixed summation order: two calls, the same bits
    again = torch.ops.mi355ppo.distill_loss_value_grad(*args, a_s, l_s)
    assert all(torch.equal(x, y) for x, y in zip((la, ll, dmu, dlat), again))


_GOLDEN = []


def _golden():
    if not _GOLDEN:
        _GOLDEN.append(lr.load_latent_golden())
    return _GOLDEN[0]


def _agent(latent_loss, action_scale=1.0, latent_scale=1.0):
    """ExtrinsicAdapt on the golden's buffer, permutation and weights.  latent_loss: True | False | None = the key absent."""
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    G, sd, teacher = _golden()
    n, T, E = [int(x) for x in G[f"{lr.TAG}/flags"][:3]]
    cfg = default_config(num_envs=n, horizon_length=T, rl_device=DEV, mini_epochs=E, obs_info=True, tactile_info=False,
                         pcl_info=False, img_info=False, seg_info=False, num_points=8)
    cfg.offline_train.only_bc = False
    cfg.offline_train.train.action_scale, cfg.offline_train.train.latent_scale = action_scale, latent_scale
    if latent_loss is None:
        del cfg.offline_train.train["latent_loss"]
    else:
        cfg.offline_train.train.latent_loss = latent_loss
    agent = ExtrinsicAdapt(SyntheticInsertionEnv(n, device=DEV), None, cfg)
    assert agent.latent_loss is bool(latent_loss)
    agent.agent.load_state_dict(teacher)
    model = agent.student.model
    assert [str(k) for k in G[f"{lr.TAG}/keys"]] == list(model.state_dict().keys())
    model.load_state_dict(sd)
    for m in model.modules():      # dropout off, as in the golden run
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    for k in ("n_obs", "latent_gt", "teacher_actions", "n_student_obs"):
        agent.storage.storage_dict[k].copy_(torch.from_numpy(G[f"{lr.TAG}/in/{k}"]))
    agent.storage.indices.copy_(torch.from_numpy(G[f"{lr.TAG}/perm"]))
    agent.storage.prepare_training()
    agent.set_student_train()
    return agent


def _update(agent):
    grad0 = {}

    def probe(step, m):
        if step == 0:
            grad0.update({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.requires_grad and p.grad is not None})

    agent.grad_probe = probe
    a_losses, l_losses = agent.update()
    torch.cuda.synchronize()
    return grad0, float(a_losses[0]), float(l_losses[0])


def _check_case(case, grad0, loss_action, loss_latent):
    G = _golden()[0]
    pre = f"{lr.TAG}/case{case}/"
    print(f"case {case}: loss_action {loss_action:.6f} (reference {float(G[pre + 'loss_action']):.6f}), loss_latent "
          f"{loss_latent:.6f} (reference {float(G[pre + 'loss_latent']):.6f})")
    np.testing.assert_allclose(loss_action, float(G[pre + "loss_action"]), rtol=2e-4)
    np.testing.assert_allclose(loss_latent, float(G[pre + "loss_latent"]), rtol=2e-4)
    names = [k[len(pre) + 6:] for k in G.files if k.startswith(pre + "grad0/")]
    assert len(names) >= 10 and set(names) <= set(grad0)
    gmax = max(np.abs(G[pre + f"grad0/{n}"]).max() for n in names)
    for n in names:
        ref, noise = G[pre + f"grad0/{n}"], float(G[pre + f"grad0_ref_noise/{n}"])
        np.testing.assert_allclose(grad0[n].cpu().numpy(), ref, atol=max(1e-3 * np.abs(ref).max(), 1e-6 * gmax, 4 * noise),
                                   rtol=1e-3, err_msg=f"case {case} grad0 {n}")


def test_trainer_with_the_switch_off_is_the_reference_live_loss():
    """latent_loss False / absent: the (1, 0) case whatever latent_scale says, and the two spellings give the same bits"""
    off = _agent(False, 1.0, 1.0)
    grad0, la, ll = _update(off)
    _check_case(0, grad0, la, ll)
    absent = _agent(None, 1.0, 1.0)
    _update(absent)
    for (n, a), (_, b) in zip(off.student.model.state_dict().items(), absent.student.model.state_dict().items()):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("case", [1, 2])
def test_trainer_with_the_latent_term_matches_the_reference(case):
    G = _golden()[0]
    a_s, l_s = [float(v) for v in G[f"{lr.TAG}/scales"][case]]
    agent = _agent(True, a_s, l_s)
    frozen = agent.agent.flat_params.clone()
    grad0, la, ll = _update(agent)
    _check_case(case, grad0, la, ll)
    assert torch.equal(frozen, agent.agent.flat_params)             # the teacher did not move


def test_latent_loss_with_only_bc_is_refused():
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device=DEV, mini_epochs=2, obs_info=True, num_points=8)
    cfg.offline_train.only_bc = True
    cfg.offline_train.train.latent_loss = True
    with pytest.raises(ValueError, match="only_bc"):
        ExtrinsicAdapt(SyntheticInsertionEnv(8, device=DEV), None, cfg)
    cfg.offline_train.only_bc = False
    cfg.offline_train.train.latent_loss = "yes"
    with pytest.raises(ValueError, match="latent_loss"):
        ExtrinsicAdapt(SyntheticInsertionEnv(8, device=DEV), None, cfg)
