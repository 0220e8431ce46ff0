"""The packed teacher cfg has one decoder (csrc/teacher_cfg.h behind igi_teacher_cfg_unpack), no GPU: every mode
combination round-trips through it, the fake kernels of the latent ops size their outputs from the decoded cfg and the
library's two width queries -- with the schedule's extra int in the list too --, and the stand-alone checker of the decoder
builds under ASan + UBSan and passes."""
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(obs_dim=15, priv_dim=64, act_dim=6, units=[510, 256, 126], priv_units=[256, 128, 8], num_envs=64, horizon=8,
             mini_epochs=4)
ADA = dict(lr_schedule="adaptive", kl_threshold=0.004)
MODES = {
    "plain": dict(),
    "shared": dict(shared_parameters=True),
    "contacts": dict(contact_points=37, contact_emb=16),
    "only_contact": dict(contact_points=37, contact_emb=8, only_contact=True),
}
CASES = [(m, a) for m in MODES for a in (False, True)]
IDS = [m + ("+adaptive" if a else "") for m, a in CASES]


def _cfg(mode, adaptive):
    from isaacgyminsertion_amd.teacher_native import make_cfg
    return make_cfg(**SHAPE, **MODES[mode], **(ADA if adaptive else {}))[0]


@pytest.mark.parametrize("mode,adaptive", CASES, ids=IDS)
def test_every_mode_round_trips(mode, adaptive):
    from isaacgyminsertion_amd import _lib, ops
    c = _cfg(mode, adaptive)
    icfg, fcfg = ops.pack_cfg(c)
    assert bytes(ops._unpack_cfg(icfg, fcfg)) == bytes(c)
    # under the early-stopping tail the cfg is the same one, and the decoder counts the steps of the stop record
    stop = torch.zeros(_lib.stop_state_words(16), dtype=torch.int32)
    i2, f2, _ = ops.pack_stop(icfg, fcfg, [], 0.004, stop)
    ks = _lib.KlStop()
    back, steps = ops._decode(i2, f2, ks)
    assert bytes(back) == bytes(c) and steps == 4 * 4 and (ks.kl_early_stop, ks.kl_threshold, ks.stop_state) == (1, 0.004, None)
    with pytest.raises(RuntimeError, match="teacher cfg: expected"):      # no stop record: the tail is a wrong length
        ops._unpack_cfg(i2, f2)


@pytest.mark.parametrize("mode,adaptive", CASES + [("contacts8", False), ("contacts8", True)], ids=IDS + ["contacts8", "contacts8+adaptive"])
def test_fake_kernels_size_the_latent_from_the_cfg(mode, adaptive):
    """Latent width W = contact_emb + (0 if only_contact else priv_units[-1]), priv_units[-1] without contacts; saved width
    = the actor's layer widths, each rounded up to 4.  contacts + adaptive: 24; shared + adaptive: 8."""
    from isaacgyminsertion_amd import ops
    from isaacgyminsertion_amd.teacher_native import make_cfg
    from torch._subclasses.fake_tensor import FakeTensorMode
    if mode == "contacts8":
        c = make_cfg(**SHAPE, contact_points=37, contact_emb=8, **(ADA if adaptive else {}))[0]
    else:
        c = _cfg(mode, adaptive)
    icfg, fcfg = ops.pack_cfg(c)
    lat = SHAPE["priv_units"][-1]
    W = c.contact_emb + (0 if c.only_contact else lat) if c.contact_points else lat
    assert W == {"plain": 8, "shared": 8, "contacts": 24, "only_contact": 8, "contacts8": 16}[mode]
    saved_w = sum((u + 3) // 4 * 4 for u in SHAPE["units"])
    assert saved_w == 512 + 256 + 128
    rows = 7
    o = torch.ops.mi355ppo
    with FakeTensorMode():
        state = [torch.empty(1)] * (17 if adaptive else 16)
        obs, priv, contacts = torch.empty(rows, 15), torch.empty(rows, 64), torch.empty(rows, 37)
        mu, val, latent = o.actor_critic_infer_contacts(state, icfg, fcfg, obs, priv, contacts, True, True)
        assert (mu.shape, val.shape, latent.shape) == ((rows, 6), (rows, 1), (rows, W))
        assert o.actor_critic_infer_contacts(state, icfg, fcfg, obs, priv, contacts, True, False)[2].shape == (0, W)
        mu, saved = o.actor_latent_fwd(state, icfg, fcfg, obs, torch.empty(rows, W), True)
        assert (mu.shape, saved.shape) == ((rows, 6), (rows, saved_w))
        assert o.actor_latent_bwd(state, icfg, fcfg, saved, torch.empty(rows, 6)).shape == (rows, W)
        mu, val, latent = o.actor_critic_infer(state, icfg, fcfg, obs, priv, True, True)
        assert (mu.shape, val.shape, latent.shape) == ((rows, 6), (rows, 1), (rows, lat))


def test_ops_hold_no_second_decoder():
    src = open(os.path.join(ROOT, "isaacgyminsertion_amd", "ops.py")).read()
    body = src.split("def _decode(")[1]                 # behind pack_cfg; pack_stop appends, it does not index
    assert "icfg[" not in body and "IGI_MAX_LAYERS" not in body
    cpp = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "torch_ops.cpp")).read()
    assert "2 * M" not in cpp and cpp.count("igi_teacher_cfg_unpack(") == 1


def test_decoder_checker_passes_under_sanitizers(tmp_path):
    """tools/teacher_cfg_check.cpp: host code with its own main and the sanitizer runtimes linked into it, so nothing is
    preloaded and whatever the environment preloads does not matter."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "teacher_cfg_check")
    subprocess.run([gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", os.path.join(ROOT, "tools", "teacher_cfg_check.cpp"), "-o", exe], check=True,
                   cwd=ROOT, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("teacher_cfg_check:") and r.stdout.rstrip().endswith(" 0 bad")
