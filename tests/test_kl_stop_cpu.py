"""KL early stopping, what needs no GPU: the cases' margin conditions on the oracle's own estimator sequence
(tests/kl_stop_cases.py), the list-slicing helper against hand-made statistics rows, configuration parsing and refusals,
the C boundary (header, exports, ctypes binding) and the packing of the stop record behind the op lists -- lists of
today's length mean "off"."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import kl_stop_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_margins(name):
    ref = K.case_oracle(name)
    print(f"{name}: stop {ref['stop']}, 1.5 thr {1.5 * ref['thr']:.4e}, estimator {ref['approx32']}, "
          f"max |fp32 - float64| {np.abs(ref['approx32'] - ref['approx64']).max():.3e}")
    K.assert_margins(name, ref)
    s = ref["stop"]
    n_eval = len(ref["approx32"])
    if ref["stop"] is None:
        assert n_eval == len(ref["a_losses"])
        return
    # the lists as the reference's breaks leave them: losses s, entropies and step KLs s + 1
    assert (n_eval, len(ref["a_losses"]), len(ref["entropies"]), len(ref["step_lr"])) == (s + 1, s, s + 1, s)
    assert ref["idx_stop"] is not None


def test_adaptive_case_runs_the_scheduler_once_more():
    ref = K.case_oracle("adaptive")
    K.assert_margins("adaptive", ref)
    s = ref["stop"]
    E_seen = s // 4 + 1
    assert len(ref["lrs"]) == len(ref["kls"]) == E_seen == 2
    assert ref["lrs"][0] == 2.5e-4 * 1.5 and ref["lrs"][1] == ref["lrs"][0]
    # the last KL is the fp32 mean over the partial mini-epoch
    part = torch.tensor(ref["step_kls"][4:s + 1], dtype=torch.float32).mean().item()
    assert ref["kl_seen"][-1] == part
    assert np.all(ref["step_lr"][:4] == 2.5e-4) and np.all(ref["step_lr"][4:] == ref["lrs"][0])


def test_slice_update_lists():
    from isaacgyminsertion_amd.teacher_native import slice_update_lists
    E, n_mb = 3, 4
    rows = torch.arange(E * n_mb * 8, dtype=torch.float32).reshape(E * n_mb, 8)
    rows[7:, :] = float("nan")          # rows behind the stop are unspecified: the helper must never read them
    rows[6, [0, 1, 2, 5, 6, 7]] = float("nan")   # at the stop step only slots 3 and 4 were written
    a, c, b, ent, kls, g = slice_update_lists(rows, E, n_mb, 6)
    assert [len(x) for x in (a, c, b, ent, kls, g)] == [6, 6, 6, 7, 2, 6]
    assert torch.equal(torch.stack(a), rows[:6, 0]) and torch.equal(torch.stack(c), rows[:6, 1])
    assert torch.equal(torch.stack(b), rows[:6, 2]) and torch.equal(torch.stack(g), rows[:6, 6])
    assert torch.equal(torch.stack(ent), rows[:7, 3])
    assert kls[0] == rows[0:4, 4].mean() and kls[1] == rows[4:7, 4].mean()
    assert all(torch.isfinite(torch.stack(x)).all() for x in (a, c, b, ent, kls, g))
    # the first step of a mini-epoch: one more KL entry, of that step alone
    a, c, b, ent, kls, g = slice_update_lists(rows, E, n_mb, 4)
    assert [len(x) for x in (a, ent, kls)] == [4, 5, 2] and kls[1] == rows[4, 4]
    # the update's first step: nothing was applied
    a, c, b, ent, kls, g = slice_update_lists(rows, E, n_mb, 0)
    assert [len(x) for x in (a, c, b, ent, kls, g)] == [0, 0, 0, 1, 1, 0] and kls[0] == rows[0, 4]
    # no stop: everything, E means
    full = torch.arange(E * n_mb * 8, dtype=torch.float32).reshape(E * n_mb, 8)
    a, c, b, ent, kls, g = slice_update_lists(full, E, n_mb, None)
    assert [len(x) for x in (a, c, b, ent, kls, g)] == [12, 12, 12, 12, 3, 12]
    assert torch.equal(torch.stack(kls), full[:, 4].reshape(E, n_mb).mean(1))
    for bad in (12, -1, 13):
        with pytest.raises(ValueError):
            slice_update_lists(full, E, n_mb, bad)


def test_rule_is_strict_and_in_double():
    from isaacgyminsertion_amd.teacher_native import kl_stop_rule
    thr = 4e-3
    assert not kl_stop_rule(1.5 * thr, thr) and kl_stop_rule(np.nextafter(1.5 * thr, 1.0), thr)
    f = np.float32(1.5 * thr)            # the fp32 estimator is widened, the limit is not narrowed
    assert kl_stop_rule(f, thr) == (float(f) > 1.5 * thr)


def test_parsing_and_refusals():
    from isaacgyminsertion_amd.algo.ppo.frozen_ppo import PPO
    from isaacgyminsertion_amd.teacher_native import parse_kl_early_stop
    from isaacgyminsertion_amd.train import build_config
    from isaacgyminsertion_amd.utils.config import default_config
    assert parse_kl_early_stop(None) is False and parse_kl_early_stop(False) is False and parse_kl_early_stop(True) is True
    for bad in ("True", "yes", 1, 0, 1.0, [True]):
        with pytest.raises(ValueError):
            parse_kl_early_stop(bad)
    cfg = default_config()
    assert cfg.train.ppo.kl_early_stop is False and PPO.parse_kl_early_stop(cfg.train.ppo) is False
    assert PPO.parse_kl_early_stop({"kl_threshold": 0.02}) is False             # key absent
    assert build_config(overrides=["train.ppo.kl_early_stop=True"]).train.ppo.kl_early_stop is True
    assert PPO.parse_kl_early_stop(build_config(overrides=["train.ppo.kl_early_stop=True"]).train.ppo) is True
    with pytest.raises(ValueError):
        build_config(overrides=["train.ppo.kl_early_stop=sometimes"])
    with pytest.raises(ValueError):
        build_config(overrides=["train.ppo.kl_early_stop=1"])
    with pytest.raises(ValueError):
        PPO.parse_kl_early_stop({"kl_early_stop": True, "kl_threshold": 0.0})
    assert PPO.parse_kl_early_stop({"kl_early_stop": True, "kl_threshold": 0.02, "multi_gpu": True}) is True


def test_header_exports_and_binding_agree():
    from isaacgyminsertion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "igi_ppo.h")).read()
    rec = re.search(r"typedef struct igi_kl_stop \{(.*?)\} igi_kl_stop;", hdr, re.S).group(1)
    fields = re.findall(r"(int32_t\*?|double)\s+(\w+);", rec)
    assert fields == [("int32_t", "kl_early_stop"), ("double", "kl_threshold"), ("int32_t*", "stop_state")]
    assert [f[0] for f in _lib.KlStop._fields_] == [n for _, n in fields]
    assert (_lib.KlStop.kl_early_stop.offset, _lib.KlStop.kl_threshold.offset, _lib.KlStop.stop_state.offset,
            C.sizeof(_lib.KlStop)) == (0, 8, 16, 24)
    assert "#define IGI_STOP_STATE_WORDS(steps) (2 + (steps))" in hdr and _lib.stop_state_words(16) == 18
    # the stop record rides beside the two structs: their layout and the ABI version are the parent's
    assert f"#define IGI_ABI_VERSION {_lib.ABI_VERSION}" in hdr
    assert [f[0] for f in _lib.TeacherCfg._fields_][-1] == "lr_max" and [f[0] for f in _lib.TeacherState._fields_][-1] == "lr_state"
    capi = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "igi_capi.hip")).read()
    cpp = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "torch_ops.cpp")).read()
    for fn in ("igi_teacher_update_dp_ks", "igi_teacher_update_dp_rccl_ks"):
        assert re.search(rf"\bint {fn}\(", hdr) and re.search(rf"\bint {fn}\(", capi), fn
        assert fn in _lib._EXPORTS and _lib._EXPORTS[fn][1].count(C.POINTER(_lib.KlStop)) == 1, fn
    for fn in ("igi_teacher_fwd_bwd_ks", "igi_teacher_apply_ks", "igi_teacher_update_ks"):
        assert re.search(rf"\bint {fn}\(", hdr) and re.search(rf"\bint {fn}\(", capi), fn
        assert fn in _lib._EXPORTS and _lib._EXPORTS[fn][1].count(C.POINTER(_lib.KlStop)) == 1, fn
        assert fn in cpp, fn
    assert "IGI_STOP_STATE_WORDS(steps)" in cpp


def test_library_exports_the_entry_points():
    from isaacgyminsertion_amd import _lib
    L = _lib.lib()          # resolves every name of _EXPORTS
    for fn in ("igi_teacher_fwd_bwd_ks", "igi_teacher_apply_ks", "igi_teacher_update_ks"):
        assert getattr(L, fn).argtypes is not None


def test_lists_of_todays_length_mean_off():
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.teacher_native import make_cfg
    M = _lib.IGI_MAX_LAYERS
    shape = dict(obs_dim=15, priv_dim=64, act_dim=6, units=[512, 256, 128], priv_units=[256, 128, 8], num_envs=64,
                 horizon=8, mini_epochs=4)
    plain, _ = make_cfg(**shape)
    ada, _ = make_cfg(**shape, lr_schedule="adaptive", kl_threshold=0.02)     # the tail's threshold below: one value for both
    state = [torch.zeros(1)] * 16
    for cfg, n_state in ((plain, 16), (ada, 17)):
        icfg, fcfg = ops.pack_cfg(cfg)
        st = [torch.zeros(1)] * n_state
        got = ops._split_stop(st, icfg, fcfg)
        assert got[3] is None and got[0] is st and got[1] is icfg and got[2] is fcfg
        # the tail: one int, one float, one tensor, behind everything else
        stop = torch.zeros(_lib.stop_state_words(4 * 4), dtype=torch.int32)
        i2, f2, s2 = ops.pack_stop(icfg, fcfg, st, 0.02, stop)
        assert i2 == icfg + [1] and f2 == fcfg + [0.02] and len(s2) == n_state + 1 and s2[-1] is stop
        assert len(f2) in (13, 16) and len(fcfg) in (12, 15)
        with pytest.raises(RuntimeError, match="stop_state"):      # a host tensor: there is no CPU path
            ops._split_stop(s2, i2, f2)
        for bad_i, bad_f in ((icfg + [0], f2), (icfg + [2], f2), (i2, fcfg + [0.0]), (i2, fcfg + [-1.0])):
            with pytest.raises(RuntimeError, match="early-stopping tail"):
                ops._split_stop(s2, bad_i, bad_f)
    icfg, fcfg = ops.pack_cfg(plain)
    assert (len(icfg), len(fcfg), len(state)) == (8 + 2 * M, 12, 16)
    assert bytes(ops._unpack_cfg(icfg, fcfg)) == bytes(plain)

