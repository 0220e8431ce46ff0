"""The learning-rate schedule's host side, no GPU: cfg packing (a fixed-schedule cfg packs exactly as a cfg built
without the new arguments; adaptive appends one int and three floats), the trainer's parsing of train.ppo.lr_schedule,
and the device rule -- restated in Python doubles by teacher_native.adaptive_lr_rule, line for line what k_lr_schedule
computes -- against AdaptiveScheduler.update on a grid that holds both decision boundaries exactly."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import lr_schedule_cases as L

SHAPE = dict(obs_dim=15, priv_dim=64, act_dim=6, units=[512, 256, 128], priv_units=[256, 128, 8], num_envs=64, horizon=8,
             mini_epochs=4)


def test_fixed_cfg_packs_as_before_and_adaptive_appends():
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.teacher_native import make_cfg
    M = _lib.IGI_MAX_LAYERS
    plain, _ = make_cfg(**SHAPE)
    fixed, _ = make_cfg(**SHAPE, lr_schedule="fixed", kl_threshold=0.004, lr_min=1e-5, lr_max=1e-3)
    assert bytes(plain) == bytes(fixed)                       # "fixed" leaves all four schedule fields zero
    assert (fixed.lr_schedule, fixed.kl_threshold, fixed.lr_min, fixed.lr_max) == (0, 0.0, 0.0, 0.0)
    icfg, fcfg = ops.pack_cfg(fixed)
    assert ops.pack_cfg(plain) == (icfg, fcfg) and len(icfg) == 8 + 2 * M and len(fcfg) == 12
    ada, _ = make_cfg(**SHAPE, lr_schedule="adaptive", kl_threshold=0.004, lr_min=1e-5, lr_max=1e-3)
    i2, f2 = ops.pack_cfg(ada)
    assert i2 == icfg + [1] and f2 == fcfg + [0.004, 1e-5, 1e-3]
    back = ops._unpack_cfg(i2, f2)
    assert bytes(back) == bytes(ada)
    assert bytes(ops._unpack_cfg(icfg, fcfg)) == bytes(plain)
    # with contacts the schedule fields still come last
    ct, _ = make_cfg(**SHAPE, contact_points=37, contact_emb=8, lr_schedule="adaptive", kl_threshold=0.01)
    i3, f3 = ops.pack_cfg(ct)
    assert len(i3) == 12 + 2 * M and i3[-4:] == [37, 8, 0, 1] and f3[12:] == [0.01, 1e-6, 1e-2]
    assert bytes(ops._unpack_cfg(i3, f3)) == bytes(ct)
    # the struct the library reads: the new fields behind only_contact, the rate buffer behind workspace_bytes
    names = [f[0] for f in _lib.TeacherCfg._fields_]
    assert names[-4:] == ["lr_schedule", "kl_threshold", "lr_min", "lr_max"] and names[-5] == "only_contact"
    assert _lib.TeacherCfg.kl_threshold.offset % 8 == 0 and C.sizeof(_lib.TeacherCfg) == _lib.TeacherCfg.lr_max.offset + 8
    assert [f[0] for f in _lib.TeacherState._fields_][-2:] == ["workspace_bytes", "lr_state"]
    assert _lib.lr_state_doubles(4) == 10 and _lib.ABI_VERSION == 6
    for bad in (dict(kl_threshold=0.0), dict(lr_min=0.0), dict(lr_min=1e-2, lr_max=1e-3)):
        with pytest.raises(ValueError):
            make_cfg(**SHAPE, lr_schedule="adaptive", **bad)
    with pytest.raises(RuntimeError):
        ops._unpack_cfg(icfg + [2], fcfg + [0.004, 1e-5, 1e-3])
    with pytest.raises(RuntimeError):
        ops._unpack_cfg(icfg + [1], fcfg)                     # the int without its floats


def test_header_binding_and_registration_agree():
    import os
    import re
    from isaacgyminsertion_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "igi_ppo.h")).read()
    assert f"#define IGI_ABI_VERSION {_lib.ABI_VERSION}" in hdr
    cfg = re.search(r"typedef struct igi_teacher_cfg \{(.*?)\} igi_teacher_cfg;", hdr, re.S).group(1)
    assert re.search(r"only_contact;.*int32_t lr_schedule;\s*double kl_threshold, lr_min, lr_max;\s*$", cfg, re.S)
    st = re.search(r"typedef struct igi_teacher_state \{(.*?)\} igi_teacher_state;", hdr, re.S).group(1)
    assert re.search(r"size_t workspace_bytes;.*double\* lr_state;\s*$", st, re.S)
    assert "#define IGI_LR_STATE_DOUBLES(mini_epochs) (2 + 2 * (mini_epochs))" in hdr
    cpp = open(os.path.join(root, "isaacgyminsertion_amd", "csrc", "torch_ops.cpp")).read()
    assert "IGI_LR_STATE_DOUBLES(c.mini_epochs)" in cpp and "c.lr_schedule ? 17 : 16" in cpp


def test_trainer_parses_the_schedule():
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.train import build_config
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=64, horizon_length=8, rl_device="cpu")
    assert cfg.train.ppo.lr_schedule == "fixed" and PPO.parse_lr_schedule(cfg.train.ppo) == "fixed"
    del cfg.train.ppo["lr_schedule"]                           # a config from before the key existed
    assert PPO.parse_lr_schedule(cfg.train.ppo) == "fixed"
    cfg = default_config(num_envs=64, horizon_length=8, rl_device="cpu", lr_schedule="adaptive")
    assert PPO.parse_lr_schedule(cfg.train.ppo) == "adaptive"
    assert build_config(None, ["train.ppo.lr_schedule=adaptive"]).train.ppo.lr_schedule == "adaptive"
    bad = default_config(num_envs=64, horizon_length=8, rl_device="cpu", lr_schedule="linear")
    for call in (lambda: PPO.parse_lr_schedule(bad.train.ppo), lambda: PPO(None, None, bad),
                 lambda: build_config(None, ["train.ppo.lr_schedule=linear"])):
        with pytest.raises(ValueError) as e:
            call()
        assert "'fixed'" in str(e.value) and "'adaptive'" in str(e.value) and "linear" in str(e.value)


def test_device_rule_equals_adaptive_scheduler_on_a_grid_with_both_boundaries():
    from isaacgyminsertion_amd.teacher_native import adaptive_lr_rule
    thrs = [0.001, 0.004, 0.008, 0.02, float(np.float32(0.013))]
    lrs = [1e-6, 1.2e-6, 2.5e-4, 1e-3, 3e-3, 8e-3, 1e-2]
    clamps = [(1e-6, 1e-2), (2.5e-3, 1e-2), (1e-6, 3e-4)]
    n = 0
    for thr, lr, (lo, hi) in itertools.product(thrs, lrs, clamps):
        lo_b, hi_b = 0.5 * thr, 2.0 * thr
        kls = [0.0, lo_b, hi_b, np.nextafter(lo_b, 0.0), np.nextafter(lo_b, 1.0), np.nextafter(hi_b, 0.0),
               np.nextafter(hi_b, 1.0), 0.1 * thr, thr, 10 * thr,
               # the device compares (double)(float)kl: fp32 neighbours of the boundaries
               float(np.float32(lo_b)), float(np.nextafter(np.float32(lo_b), np.float32(0))),
               float(np.nextafter(np.float32(hi_b), np.float32(1)))]
        for kl in kls:
            kl = float(kl)
            want = L.rule(lr, kl, thr, lo, hi)
            assert adaptive_lr_rule(lr, kl, thr, lo, hi) == want, (thr, lr, lo, hi, kl)
            n += 1
        # strict inequalities: a KL exactly on a boundary moves nothing
        assert adaptive_lr_rule(lr, hi_b, thr, lo, hi) == lr and adaptive_lr_rule(lr, lo_b, thr, lo, hi) == lr
        assert adaptive_lr_rule(lr, float(np.nextafter(hi_b, 1.0)), thr, lo, hi) == max(lr / 1.5, lo)
        assert adaptive_lr_rule(lr, float(np.nextafter(lo_b, 0.0)), thr, lo, hi) == min(lr * 1.5, hi)
    assert n == len(thrs) * len(lrs) * len(clamps) * 13


def test_case_table_holds_on_the_cpu_oracle():
    """The cases the GPU tests use, re-checked here: the decisions the issue lists and the 10 % margins."""
    for name in ("C", "C_contacts"):
        ref = L.case_oracle(name)
        L.assert_margins(ref)
        assert L.decisions(L.CASES[name][3], ref["lrs"][0]) == L.EXPECTED[name]
