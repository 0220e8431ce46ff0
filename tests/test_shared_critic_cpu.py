"""Teacher with a shared actor-critic trunk (train.ppo.shared_parameters), everything that needs no GPU: the shared
restatement (tests/shared_critic_ref.py) pinned to goldens captured from the reference's own PPO, the seeded
initialisation and state_dict layout of ActorCriticSplit, the C struct and parameter layout, the packed cfg's round trips
through both decoders, and the combinations that stay refused."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import shared_critic_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS, PRIV_UNITS = [64, 32, 16], [32, 16, 8]
DEFAULT_UNITS, DEFAULT_PRIV_UNITS = [512, 256, 128], [256, 128, 8]


@pytest.mark.parametrize("case", ["small", "default"])
def test_shared_restatement_matches_reference(case):
    """tests/test_oracle_teacher.py's checks and tolerances, on the shared goldens."""
    torch.set_num_threads(1)
    g, meta, init = sr.load(case)
    shapes = sr.param_shapes(15, 64, 6, meta["units"], meta["priv_units"])
    assert list(shapes.keys()) == list(init.keys()) and len(init) == 17
    assert all(tuple(init[k].shape) == s for k, s in shapes.items())
    orc = sr.SharedTeacherOracle(init, torch.from_numpy(g["perm"]), meta["num_envs"], meta["horizon"],
                                 meta["mini_epochs"], meta["units"], meta["priv_units"])
    from tests.golden_io import rollout
    for u in range(meta["n_updates"]):
        d = orc.prepare(rollout(g, u))
        np.testing.assert_allclose(orc.returns_raw.numpy(), g[f"u{u}/returns_raw"], rtol=0, atol=0)
        np.testing.assert_allclose(d["advantages"].numpy(), g[f"u{u}/advantages"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(d["values"].numpy(), g[f"u{u}/values_norm"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(d["returns"].numpy(), g[f"u{u}/returns_norm"], rtol=1e-6, atol=1e-6)
        vms = g[f"u{u}/vms_after_tail"]
        np.testing.assert_allclose([orc.rms_val.mean.item(), orc.rms_val.var.item(), orc.rms_val.count.item()],
                                   vms, rtol=1e-12)
        st = orc.update(record_grads=1)
        np.testing.assert_allclose(st["grads"][0].numpy(), g[f"u{u}/grad_step0"], rtol=1e-5, atol=1e-8)
        for name in ["a_losses", "c_losses", "b_losses", "entropies", "kls", "grad_total_norms", "param_norms"]:
            got = np.array([x.item() for x in st[name]], dtype=np.float32)
            np.testing.assert_allclose(got, g[f"u{u}/{name}"], rtol=2e-5, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(orc.flat_params().numpy(), g[f"u{u}/params_after"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(orc.data["mus"].numpy(), g[f"u{u}/mus_after"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(orc.data["sigmas"].numpy(), g[f"u{u}/sigmas_after"], rtol=1e-6)
        for nm, rs in [("running_mean_std", orc.rms_obs), ("priv_mean_std", orc.rms_priv),
                       ("value_mean_std", orc.rms_val)]:
            np.testing.assert_allclose(rs.mean.numpy(), g[f"u{u}/{nm}/running_mean"], rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(rs.var.numpy(), g[f"u{u}/{nm}/running_var"], rtol=1e-10)
            assert rs.count.item() == g[f"u{u}/{nm}/count"].item()


def test_swapped_forward_is_put_back():
    from oracle import teacher as ot
    keep = ot.forward_train
    g, meta, init = sr.load("small")
    orc = sr.SharedTeacherOracle(init, torch.from_numpy(g["perm"]), meta["num_envs"], meta["horizon"],
                                 meta["mini_epochs"], meta["units"], meta["priv_units"])
    from tests.golden_io import rollout
    orc.prepare(rollout(g, 0))
    orc.update(max_steps=1)
    assert ot.forward_train is keep


def _kwargs(**over):
    kw = dict(actor_units=UNITS, actions_num=6, input_shape=(15,), priv_mlp_units=PRIV_UNITS, priv_info_dim=64,
              priv_info=True, gt_contacts_info=False, only_contact=False, contacts_mlp_units=[8],
              num_contact_points=37, shared_parameters=True, vt_policy=False)
    kw.update(over)
    return kw


def _reference_recipe():
    """The reference's construction order and initialisation with shared_parameters (models_split.py:27-117): env_mlp,
    actor_mlp, value, mu -- no critic_mlp, so value's and mu's orthogonal draws follow actor_mlp's directly."""
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
    m.actor_mlp = nn.Module()
    m.actor_mlp.mlp = mlp(UNITS, 15 + PRIV_UNITS[-1])
    m.value = layer_init(nn.Linear(UNITS[-1], 1), std=1.0)
    m.mu = layer_init(nn.Linear(UNITS[-1], 6), std=0.01)
    for mod in m.modules():
        if isinstance(mod, nn.Linear):
            nn.init.zeros_(mod.bias)
    return m.state_dict()


def test_shared_state_dict_is_the_reference_layout():
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    torch.manual_seed(42)
    m = ActorCriticSplit(_kwargs())
    torch.manual_seed(42)
    ref = _reference_recipe()
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys()) and len(sd) == 17
    assert not hasattr(m, "critic_mlp") and not any(k.startswith("critic_mlp") for k in sd)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
        np.testing.assert_allclose(sd[k].numpy(), ref[k].numpy(), atol=2e-6, err_msg=k)
    base = m.flat_params.data_ptr()                       # every parameter is a view of the one flat vector
    for p in m.parameters():
        assert base <= p.data_ptr() < base + m.flat_params.numel() * 4
    # a reference-written state_dict (no critic_mlp.* keys) loads strictly, and the views stay views
    ck, units, priv_units = sr.load_ckpt()
    m2 = ActorCriticSplit(_kwargs(actor_units=units, priv_mlp_units=priv_units))
    m2.load_state_dict(ck["model"])
    assert list(m2.state_dict().keys()) == list(ck["model"].keys())
    for k, v in ck["model"].items():
        assert torch.equal(m2.state_dict()[k], v), k
    assert m2.mu.weight.data_ptr() >= m2.flat_params.data_ptr()


def test_shared_param_layout():
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.teacher_native import (make_cfg, param_layout, teacher_param_names, teacher_param_shapes)
    plain, _ = make_cfg(15, 64, 6, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, 4096, 32, 8)
    cfg, _ = make_cfg(15, 64, 6, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, 4096, 32, 8, shared_parameters=True)
    assert (plain.shared_parameters, cfg.shared_parameters) == (0, 1)
    total, layout = param_layout(cfg)
    _, lay0 = param_layout(plain)
    shapes = teacher_param_shapes(15, 64, 6, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, shared_parameters=True)
    assert list(shapes) == teacher_param_names(3, 3, shared_parameters=True) == list(sr.param_shapes(15, 64, 6, DEFAULT_UNITS, DEFAULT_PRIV_UNITS))
    assert len(layout) == len(shapes) == 17 and len(lay0) == 23
    assert all(int(np.prod(sh)) == sz for sh, (_, sz) in zip(shapes.values(), layout))
    assert sum(s for _, s in layout) == 227989 and sum(s for _, s in lay0) == 404501
    assert all(off % 4 == 0 for off, _ in layout)
    offs = [o for o, _ in layout]
    assert offs == sorted(offs) and total >= offs[-1] + layout[-1][1]
    # everything ahead of the (absent) critic block sits where it sat; the heads follow the actor's last bias directly
    n_front = 1 + 6 + 6
    assert layout[:n_front] == lay0[:n_front]
    assert layout[n_front][0] == lay0[n_front][0]          # value.weight where critic_mlp.mlp.0.weight began
    # the switch took _pad0's slot: the struct's size and every other offset are unchanged, zero means off
    T = _lib.TeacherCfg
    assert ctypes.sizeof(T) == 184 and _lib.IGI_MAX_LAYERS == 4      # the size it had with _pad0 in that slot
    assert T.shared_parameters.offset == T.mini_epochs.offset + 4 == 64 and T.gamma.offset == 72
    assert T().shared_parameters == 0
    L = _lib.lib()
    assert 0 < L.igi_teacher_workspace_bytes(ctypes.byref(cfg)) < L.igi_teacher_workspace_bytes(ctypes.byref(plain))
    bad, _ = make_cfg(15, 64, 6, DEFAULT_UNITS, DEFAULT_PRIV_UNITS, 4096, 32, 8)
    bad.shared_parameters = 2
    assert L.igi_teacher_param_count(ctypes.byref(bad)) == _lib.IGI_E_BADARG
    # the four gradient ranges of the two-phase update cover every parameter exactly once; both critic ranges are empty
    off, ln = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    assert L.igi_teacher_grad_buckets(ctypes.byref(cfg), off, ln) == 4
    assert ln[1] == 0 and ln[3] == 0
    cover = np.zeros(total, dtype=np.int32)
    for o, n in zip(off, ln):
        cover[o:o + n] += 1
    assert (cover == 1).all()
    assert off[0] == layout[9][0] and off[2] == 0 and ln[2] == off[0]   # the cut: ahead of actor_mlp.mlp.2.weight


def test_shared_cfg_round_trips():
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.teacher_native import make_cfg
    M = _lib.IGI_MAX_LAYERS
    plain, _ = make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2)
    ic0, fc0 = ops.pack_cfg(plain)
    assert len(ic0) == 8 + 2 * M and len(fc0) == 12          # the switch off packs exactly as before
    assert ops._unpack_cfg(ic0, fc0).shared_parameters == 0
    cfg, _ = make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2, shared_parameters=True)
    ic, fc = ops.pack_cfg(cfg)
    assert ic == ic0 + [1, 0] and fc == fc0
    assert ops._unpack_cfg(ic, fc).shared_parameters == 1
    # with the schedule tail, the early-stopping tail, and both
    sched, _ = make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2, shared_parameters=True, lr_schedule="adaptive",
                        kl_threshold=0.004)
    ics, fcs = ops.pack_cfg(sched)
    assert ics == ic0 + [1, 0, 1] and fcs == fc0 + [0.004, 1e-6, 1e-2]
    back = ops._unpack_cfg(ics, fcs)
    assert (back.shared_parameters, back.lr_schedule, back.kl_threshold) == (1, 1, 0.004)
    stop_state = torch.zeros(_lib.stop_state_words(4), dtype=torch.int32)
    for i_, f_ in ((ic, fc), (ics, fcs)):
        i2, f2, st2 = ops.pack_stop(i_, f_, [torch.zeros(1)], 0.004, stop_state)
        assert i2 == i_ + [1] and f2 == f_ + [0.004] and st2[-1] is stop_state
    for bad in ([2, 0], [1, 1], [0, 0]):
        with pytest.raises(RuntimeError, match="shared-trunk fields"):
            ops._unpack_cfg(ic0 + bad, fc0)
    with pytest.raises(RuntimeError, match="teacher cfg"):
        ops._unpack_cfg(ic0 + [1], fc0)                      # 9 + 2M ints: the schedule's int without its floats


def test_shared_refusals():
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    from isaacgyminsertion_amd.teacher_native import make_cfg
    with pytest.raises(NotImplementedError, match="shared_parameters with compute_contact_gt"):
        ActorCriticSplit(_kwargs(gt_contacts_info=True))
    with pytest.raises(NotImplementedError):
        ActorCriticSplit(_kwargs(priv_info=False))
    with pytest.raises(NotImplementedError):
        ActorCriticSplit(_kwargs(vt_policy=True))
    with pytest.raises(NotImplementedError, match="shared_parameters with compute_contact_gt"):
        make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2, contact_points=37, contact_emb=8, shared_parameters=True)
    cfg, _ = make_cfg(15, 64, 6, UNITS, PRIV_UNITS, 64, 8, 2, contact_points=37, contact_emb=8)
    cfg.shared_parameters = 1                                # the library itself: IGI_E_UNSUPPORTED from make_plan
    L = _lib.lib()
    assert L.igi_teacher_param_count(ctypes.byref(cfg)) == _lib.IGI_E_UNSUPPORTED
    assert L.igi_teacher_workspace_bytes(ctypes.byref(cfg)) == 0


def test_cpp_registration_decodes_a_shared_cfg():
    """The C++ registration (csrc/torch_ops.cpp) in a child process (one process holds one registration of the namespace):
    its decoder takes the shared cfg, alone and under the schedule tail, as far as the CPU-tensor refusal behind it, and
    refuses the malformed ones by name.  (Under the early-stopping tail the op is tests/test_gpu_shared_critic.py's; the
    decoder itself takes that combination in tests/test_teacher_cfg_cpu.py.)"""
    lib = os.path.join(ROOT, "isaacgyminsertion_amd", "libigi_torch_ops.so")
    if not os.path.exists(lib):
        pytest.skip("libigi_torch_ops.so not built on this host (python -c 'import __graft_entry__ as g; g.build()')")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cpp_ops_shared_child.py"), "decode"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("shared", "shared_sched", "plain"):
        assert got[k] == "tensor", (k, got)                  # decoded; the CPU tensors behind it were refused
    assert got["field_2"] == "shared-trunk fields" and got["nine_ints"] == "teacher cfg"
