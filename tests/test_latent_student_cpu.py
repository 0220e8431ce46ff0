"""CPU-side checks of the latent student (offline_train.only_bc=False): the restatement the GPU tests measure against
(tests/latent_student_ref.py) reproduces what the reference's own modules gave -- the existing golden ``lin_latent`` of
student.npz (the reference's unmodified train_epoch: the action term alone) and the three (action_scale, latent_scale)
cases of student_latent.npz (ext_adapt.py:827 with its latent term live) --, the three new ops are registered with schemas,
fake kernels and the CPU refusal, the library exports their entry points, and the ``latent_loss`` key parses."""
import os

import numpy as np
import pytest
import torch

from tests import latent_student_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check(r, loss_action, loss_latent, grads, noise):
    np.testing.assert_allclose(float(r["loss_action"]), loss_action, rtol=1e-6)
    if loss_latent is not None:
        np.testing.assert_allclose(float(r["loss_latent"]), loss_latent, rtol=1e-6)
    assert len(grads) >= 10 and set(grads) <= set(r["grads"])
    for n, ref in grads.items():
        np.testing.assert_allclose(r["grads"][n].numpy(), ref, rtol=0, atol=max(1e-5 * np.abs(ref).max(), 4 * noise[n]),
                                   err_msg=n)


def test_restatement_reproduces_the_reference_lin_latent_golden():
    G = np.load(os.path.join(GOLDEN, "student.npz"))
    tag = "lin_latent"
    sd = {k[len(tag) + 6:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/init/")}
    teacher = {k[len(tag) + 9:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/teacher/")}
    sobs, nobs, act, lgt = lr.minibatch0(G, tag)
    assert sobs.shape[0] == 16
    r = lr.step(sd, teacher, sobs, nobs, act, lgt, 1.0, 0.0)
    names = [k[len(tag) + 7:] for k in G.files if k.startswith(f"{tag}/grad0/")]
    _check(r, float(G[f"{tag}/action_losses"][0]), None, {n: G[f"{tag}/grad0/{n}"] for n in names},
           {n: float(G[f"{tag}/grad0_ref_noise/{n}"]) for n in names})


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_reproduces_the_latent_loss_golden(case):
    G, sd, teacher = lr.load_latent_golden()
    a_s, l_s = [float(v) for v in G[f"{lr.TAG}/scales"][case]]
    assert (a_s, l_s) == ((1.0, 0.0), (1.0, 1.0), (1.3, 0.7))[case]
    sobs, nobs, act, lgt = lr.minibatch0(G, lr.TAG)
    assert sobs.shape[0] == 70
    r = lr.step(sd, teacher, sobs, nobs, act, lgt, a_s, l_s)
    pre = f"{lr.TAG}/case{case}/"
    names = [k[len(pre) + 6:] for k in G.files if k.startswith(pre + "grad0/")]
    _check(r, float(G[pre + "loss_action"]), float(G[pre + "loss_latent"]), {n: G[pre + f"grad0/{n}"] for n in names},
           {n: float(G[pre + f"grad0_ref_noise/{n}"]) for n in names})
    for k in ("mu", "latent", "dlatent"):
        ref = G[pre + k]
        np.testing.assert_allclose(r[k].numpy(), ref, rtol=0,
                                   atol=max(1e-5 * np.abs(ref).max(), 4 * float(G[pre + k + "_ref_noise"])), err_msg=k)


def test_new_ops_are_registered_with_schemas_and_fake_kernels():
    from isaacgyminsertion_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("actor_latent_fwd", "actor_latent_bwd", "distill_loss_value_grad"):
        assert name in ops.OP_NAMES
        assert str(getattr(torch.ops.mi355ppo, name).default._schema).startswith(f"mi355ppo::{name}(")
    s = str(torch.ops.mi355ppo.actor_latent_fwd.default._schema)
    assert "Tensor(a!)[] state" in s and "bool save" in s and "-> (Tensor, Tensor)" in s
    assert "-> Tensor" in str(torch.ops.mi355ppo.actor_latent_bwd.default._schema)
    s = str(torch.ops.mi355ppo.distill_loss_value_grad.default._schema)
    assert "float action_scale, float latent_scale" in s and "-> (Tensor, Tensor, Tensor, Tensor)" in s
    with FakeTensorMode():
        icfg = [15, 64, 6, 3, 48, 32, 8, 0, 3, 62, 48, 30, 0, 16, 4, 2]       # widths 62 / 48 / 30 -> 64 + 48 + 32 saved
        state = [torch.empty(1)] * 16
        mu, saved = torch.ops.mi355ppo.actor_latent_fwd(state, icfg, [0.0] * 12, torch.empty(7, 15), torch.empty(7, 8), True)
        assert mu.shape == (7, 6) and saved.shape == (7, 144) and saved.dtype == torch.float32
        mu, saved = torch.ops.mi355ppo.actor_latent_fwd(state, icfg, [0.0] * 12, torch.empty(7, 15), torch.empty(7, 8), False)
        assert mu.shape == (7, 6) and saved.shape == (0, 144)
        dl = torch.ops.mi355ppo.actor_latent_bwd(state, icfg, [0.0] * 12, torch.empty(7, 144), torch.empty(7, 6))
        assert dl.shape == (7, 8)
        la, ll, dmu, dlat = torch.ops.mi355ppo.distill_loss_value_grad(torch.empty(9, 6), torch.empty(9, 6), torch.empty(6),
                                                                       torch.empty(9, 8), torch.empty(9, 8), 1.0, 0.5)
        assert la.shape == () and ll.shape == () and dmu.shape == (9, 6) and dlat.shape == (9, 8)


def test_new_ops_refuse_cpu_tensors():
    from isaacgyminsertion_amd import ops
    from isaacgyminsertion_amd.teacher_native import make_cfg
    with pytest.raises(RuntimeError, match="HIP"):
        torch.ops.mi355ppo.distill_loss_value_grad(torch.zeros(2, 6), torch.zeros(2, 6), torch.ones(6), torch.zeros(2, 8),
                                                   torch.zeros(2, 8), 1.0, 1.0)
    cfg, _ = make_cfg(15, 64, 6, [512, 256, 128], [256, 128, 8], 64, 1, 1)
    ic, fc = ops.pack_cfg(cfg)
    state = [torch.zeros(4)] * 16
    with pytest.raises(RuntimeError, match="HIP"):
        torch.ops.mi355ppo.actor_latent_fwd(state, ic, fc, torch.zeros(2, 15), torch.zeros(2, 8), False)
    with pytest.raises(RuntimeError, match="HIP"):
        torch.ops.mi355ppo.actor_latent_bwd(state, ic, fc, torch.zeros(2, 896), torch.zeros(2, 6))


def test_library_exports_the_entry_points():
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.teacher_native import make_cfg
    import ctypes as C
    L = _lib.lib()
    for name in ("igi_actor_latent_forward", "igi_actor_latent_backward", "igi_distill_loss"):
        assert getattr(L, name) is not None
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "igi_ppo.h")).read()
    for name in ("igi_actor_latent_forward(", "igi_actor_latent_backward(", "igi_distill_loss("):
        assert name in hdr
    cfg, _ = make_cfg(15, 64, 6, [62, 48, 30], [256, 128, 8], 64, 1, 1)
    assert L.igi_actor_latent_saved_width(C.byref(cfg)) == 144
    # argument refusals that need no device: NULL pointers, a latent of another width than the teacher's
    assert L.igi_distill_loss(None, None, None, 4, 6, None, None, 8, 1.0, 1.0, None, None, None, None, None) != 0
    assert L.igi_actor_latent_forward(C.byref(cfg), None, None, None, 8, 4, None, None, None) != 0


def test_latent_loss_key_parses():
    from isaacgyminsertion_amd.utils.config import default_config, parse_latent_loss
    from isaacgyminsertion_amd.train import build_config
    assert parse_latent_loss(None) is False and parse_latent_loss(False, only_bc=True) is False
    assert parse_latent_loss(True, only_bc=False) is True
    for bad in ("yes", "True", 1, 0, 1.0, [True]):
        with pytest.raises(ValueError, match="latent_loss"):
            parse_latent_loss(bad)
    with pytest.raises(ValueError, match="only_bc"):
        parse_latent_loss(True, only_bc=True)
    assert default_config().offline_train.train.latent_loss is False
    cfg = build_config(overrides=["offline_train.only_bc=False", "offline_train.train.latent_loss=True"])
    assert cfg.offline_train.train.latent_loss is True
    with pytest.raises(ValueError, match="latent_loss"):
        build_config(overrides=["offline_train.only_bc=False", "offline_train.train.latent_loss=on_please"])
    with pytest.raises(ValueError, match="only_bc"):
        build_config(overrides=["offline_train.only_bc=True", "offline_train.train.latent_loss=True"])


def test_latent_of_the_wrong_width_names_both_widths():
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    net = ActorCriticSplit({'actions_num': 6, 'input_shape': (15,), 'actor_units': [512, 256, 128],
                            'priv_mlp_units': [256, 128, 8], 'priv_info': True, 'priv_info_dim': 64})
    assert net.latent_width == 8
    for fn in (net.act_inference, net.act_with_grad):
        with pytest.raises(ValueError, match=r"width 5 .* width 8"):
            fn({'obs': torch.zeros(3, 15), 'latent': torch.zeros(3, 5)})
