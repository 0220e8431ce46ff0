"""CPU-side checks of the teacher with ground-truth contacts (task.env.compute_contact_gt): the reference's state_dict
layout and seeded initialisation of ActorCriticSplit with a ContactAE (models_split.py:41-55, 78-88, 108-117), the
library's parameter layout, the configurations that keep raising, and the contact kernels' resources."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNITS, PRIV_UNITS, P, E = [64, 32, 16], [32, 16, 8], 37, 8


def _kwargs(**over):
    kw = dict(actor_units=UNITS, actions_num=6, input_shape=(15,), priv_mlp_units=PRIV_UNITS, priv_info_dim=64,
              priv_info=True, gt_contacts_info=True, only_contact=False, contacts_mlp_units=[E],
              num_contact_points=P, shared_parameters=False, vt_policy=False)
    kw.update(over)
    return kw


def _reference_recipe(only_contact=False):
    """The reference's construction order and initialisation (models_split.py:27-117), restated in plain torch."""
    def layer_init(layer, std=np.sqrt(2)):
        nn.init.orthogonal_(layer.weight, std)
        nn.init.constant_(layer.bias, 0.0)
        return layer

    def mlp(units, d):
        layers = []
        for u in units:
            layers += [layer_init(nn.Linear(d, u)), nn.Tanh()]
            d = u
        return nn.Sequential(*layers)

    m = nn.Module()
    m.sigma = nn.Parameter(torch.zeros(6))
    m.env_mlp = nn.Module()
    m.env_mlp.mlp = mlp(PRIV_UNITS, 64)
    m.contact_ae = nn.Module()
    m.contact_ae.contact_enc_mlp = nn.Sequential(nn.Linear(P, 32), nn.ReLU(), nn.Linear(32, E), nn.Tanh())
    m.contact_ae.contact_dec_mlp = nn.Sequential(nn.Linear(E, 32), nn.ReLU(), nn.Linear(32, P))
    d = 15 + PRIV_UNITS[-1] + (0 if only_contact else E)
    for net in ("actor_mlp", "critic_mlp"):
        setattr(m, net, nn.Module())
        getattr(m, net).mlp = mlp(UNITS, d)
    m.value = layer_init(nn.Linear(UNITS[-1], 1), std=1.0)
    m.mu = layer_init(nn.Linear(UNITS[-1], 6), std=0.01)
    for mod in m.modules():
        if isinstance(mod, nn.Linear):
            nn.init.zeros_(mod.bias)
    return m.state_dict()


@pytest.mark.parametrize("only_contact", [False, True])
def test_contact_state_dict_is_the_reference_layout(only_contact):
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    torch.manual_seed(42)
    m = ActorCriticSplit(_kwargs(only_contact=only_contact))
    torch.manual_seed(42)
    ref = _reference_recipe(only_contact)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert [k for k in sd if k.startswith("contact_ae")] == [
        "contact_ae.contact_enc_mlp.0.weight", "contact_ae.contact_enc_mlp.0.bias",
        "contact_ae.contact_enc_mlp.2.weight", "contact_ae.contact_enc_mlp.2.bias",
        "contact_ae.contact_dec_mlp.0.weight", "contact_ae.contact_dec_mlp.0.bias",
        "contact_ae.contact_dec_mlp.2.weight", "contact_ae.contact_dec_mlp.2.bias"]
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
        np.testing.assert_allclose(sd[k].numpy(), ref[k].numpy(), atol=2e-6, err_msg=k)
    assert sd["contact_ae.contact_enc_mlp.0.weight"].abs().max() > 0   # torch's default init, not zeros
    # every parameter is a view of the one flat vector
    base = m.flat_params.data_ptr()
    for p in m.parameters():
        assert base <= p.data_ptr() < base + m.flat_params.numel() * 4


def test_contact_param_layout_has_the_contact_tensors():
    from isaacgyminsertion_amd.teacher_native import make_cfg, param_layout, teacher_param_shapes
    plain, _ = make_cfg(15, 64, 6, [512, 256, 128], [256, 128, 8], 4096, 32, 8)
    cfg, _ = make_cfg(15, 64, 6, [512, 256, 128], [256, 128, 8], 4096, 32, 8, contact_points=400, contact_emb=8)
    _, lay0 = param_layout(plain)
    total, layout = param_layout(cfg)
    shapes = teacher_param_shapes(15, 64, 6, [512, 256, 128], [256, 128, 8], 400, 8)
    assert len(layout) == len(shapes) == 23 + 8
    assert all(int(np.prod(sh)) == sz for sh, (_, sz) in zip(shapes.values(), layout))
    assert all(off % 4 == 0 for off, _ in layout)
    offs = [o for o, _ in layout]
    assert offs == sorted(offs) and total >= offs[-1] + layout[-1][1]
    # the trunk's first layer sees obs + priv latent + contact embedding; everything else keeps its size
    assert shapes["actor_mlp.mlp.0.weight"] == (512, 15 + 8 + 8)
    extra = 32 * 400 + 32 + 8 * 32 + 8 + 32 * 8 + 32 + 400 * 32 + 400 + 2 * 512 * 8
    assert sum(s for _, s in layout) == sum(s for _, s in lay0) + extra
    oc, _ = make_cfg(15, 64, 6, [512, 256, 128], [256, 128, 8], 4096, 32, 8, contact_points=400, contact_emb=8,
                     only_contact=True)
    assert dict(zip(teacher_param_shapes(15, 64, 6, [512, 256, 128], [256, 128, 8], 400, 8, True),
                    param_layout(oc)[1]))["actor_mlp.mlp.0.weight"][1] == 512 * 23


def test_contact_cfg_packs_only_when_on():
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.teacher_native import make_cfg
    plain, _ = make_cfg(15, 64, 6, [512, 256, 128], [256, 128, 8], 4096, 32, 8)
    ic, fc = ops.pack_cfg(plain)
    assert len(ic) == 8 + 2 * _lib.IGI_MAX_LAYERS        # a contact-free cfg packs exactly as before
    cfg, _ = make_cfg(15, 64, 6, [512, 256, 128], [256, 128, 8], 4096, 32, 8, contact_points=400, contact_emb=8)
    ic2, fc2 = ops.pack_cfg(cfg)
    assert ic2[:len(ic)] == ic and ic2[len(ic):] == [400, 8, 0] and fc2 == fc
    back = ops._unpack_cfg(ic2, fc2)
    assert (back.contact_points, back.contact_emb, back.only_contact) == (400, 8, 0)
    import ctypes
    L = _lib.lib()
    assert L.igi_teacher_workspace_bytes(ctypes.byref(cfg)) > L.igi_teacher_workspace_bytes(ctypes.byref(plain)) > 0


def test_contact_refusals():
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    from isaacgyminsertion_amd.teacher_native import make_cfg
    with pytest.raises(NotImplementedError):
        ActorCriticSplit(_kwargs(shared_parameters=True))
    with pytest.raises(NotImplementedError):
        ActorCriticSplit(_kwargs(priv_info=False))
    with pytest.raises(NotImplementedError):
        ActorCriticSplit(_kwargs(vt_policy=True))
    with pytest.raises(NotImplementedError):
        ActorCriticSplit(_kwargs(only_contact=True, contacts_mlp_units=[16]))
    with pytest.raises(NotImplementedError):
        make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2, contact_points=P, contact_emb=16, only_contact=True)
    with pytest.raises(ValueError):
        make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2, contact_points=P, contact_emb=33)


def test_extrinsic_adapt_refuses_a_contact_teacher():
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu", compute_contact_gt=True, num_points=P)
    with pytest.raises(NotImplementedError, match="contact teacher"):
        ExtrinsicAdapt(None, None, cfg)


def test_contact_kernels_do_not_spill():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = ('#include "contact.h"\n'
           'void run(const igi::ContactArgs& a, hipStream_t s) { (void)igi::contact_forward(a, s); '
           '(void)igi::contact_backward(a, s); }\n')
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "ct.hip")
        with open(f, "w") as fh:
            fh.write(src)
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-c",
                            "-I", os.path.join(ROOT, "isaacgyminsertion_amd", "csrc"),
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "x.o"), f],
                           capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    found = 0
    for b in blocks:
        name = b.split()[0]
        if "k_contact" not in name:
            continue
        found += 1
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
        vgpr = int(re.search(r"VGPRs: (\d+)", b).group(1))
        m = re.search(r"AGPRs: (\d+)", b)
        assert vgpr + (int(m.group(1)) if m else 0) <= 128, name
    assert found == 3, found
