"""Pin the CPU oracle's contact path (oracle/teacher.py: ContactAE.forward_enc in the latent, models_split.py:41-55,
166-183) against golden vectors captured from the reference's own PPO.train_epoch with compute_contact_gt
(tests/golden/make_golden_teacher_contacts.py).  Same assertions and tolerances as test_oracle_matches_reference.  CPU only."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import teacher as ot
from tests.golden_io import GOLDEN, ROLLOUT_KEYS


def _load(case):
    z = np.load(os.path.join(GOLDEN, f"teacher_contacts_{case}.npz"))
    g = {k: z[k] for k in z.files}
    N, T, E, n_up = [int(x) for x in g["meta"]]
    P, emb, oc = [int(x) for x in g["meta_contacts"]]
    meta = dict(num_envs=N, horizon=T, mini_epochs=E, n_updates=n_up, P=P, emb=emb, only_contact=bool(oc),
                units=[int(x) for x in g["units"]], priv_units=[int(x) for x in g["priv_units"]])
    init = OrderedDict((k[len("init/"):], torch.from_numpy(v)) for k, v in g.items() if k.startswith("init/"))
    return g, meta, init


@pytest.mark.parametrize("case", ["contacts", "only_contact"])
def test_oracle_contact_path_matches_reference(case):
    torch.set_num_threads(1)
    g, meta, init = _load(case)
    P, emb, oc = meta["P"], meta["emb"], meta["only_contact"]
    # parameter layout is the reference's state_dict order, contact_ae between env_mlp and actor_mlp
    shapes = ot.teacher_param_shapes(15, 64, 6, meta["units"], meta["priv_units"], P, emb, oc)
    assert list(shapes.keys()) == list(init.keys())
    assert all(tuple(init[k].shape) == s for k, s in shapes.items())
    orc = ot.TeacherOracle(init, torch.from_numpy(g["perm"]), meta["num_envs"], meta["horizon"], meta["mini_epochs"],
                           meta["units"], meta["priv_units"], contact_points=P, contact_emb=emb, only_contact=oc)
    frozen = [k for k in init if k.startswith("contact_ae.contact_dec_mlp") or (oc and k.startswith("env_mlp"))]
    assert frozen
    for u in range(meta["n_updates"]):
        ro = {k: torch.from_numpy(g[f"u{u}/in/{k}"]) for k in ROLLOUT_KEYS + ["contacts"]}
        d = orc.prepare(ro)
        np.testing.assert_allclose(orc.returns_raw.numpy(), g[f"u{u}/returns_raw"], rtol=0, atol=0)
        np.testing.assert_allclose(d["advantages"].numpy(), g[f"u{u}/advantages"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(d["values"].numpy(), g[f"u{u}/values_norm"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(d["returns"].numpy(), g[f"u{u}/returns_norm"], rtol=1e-6, atol=1e-6)
        vms = g[f"u{u}/vms_after_tail"]
        np.testing.assert_allclose([orc.rms_val.mean.item(), orc.rms_val.var.item(), orc.rms_val.count.item()],
                                   vms, rtol=1e-12)
        st = orc.update(record_grads=1)
        g0, ref0 = st["grads"][0].numpy(), g[f"u{u}/grad_step0"]
        print(f"{case} u{u} grad_step0: max |diff| {np.abs(g0 - ref0).max():.3e}, "
              f"max diff / (1e-8 + 1e-5 |ref|) {(np.abs(g0 - ref0) / (1e-8 + 1e-5 * np.abs(ref0))).max():.3f}")
        np.testing.assert_allclose(g0, ref0, rtol=1e-5, atol=1e-8)
        off = 0
        for k, v in init.items():      # grad None in the reference: zeros in the recorded flat gradient
            if k in frozen:
                assert not g0[off:off + v.numel()].any() and not ref0[off:off + v.numel()].any(), k
            off += v.numel()
        for name in ["a_losses", "c_losses", "b_losses", "entropies", "kls", "grad_total_norms",
                     "param_norms"]:
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
        adam = orc.adam_state()
        for k in frozen:               # parameter and Adam moments untouched
            assert torch.equal(orc.p[k].detach(), init[k]), k
            assert not adam[k][0].any() and not adam[k][1].any(), k


def test_oracle_default_path_ignores_the_contact_arguments():
    """contact_points = 0 (the default) is the old oracle: same shapes, same call, no contact tensors."""
    a = ot.teacher_param_shapes(15, 64, 6, [64, 32], [16, 8])
    b = ot.teacher_param_shapes(15, 64, 6, [64, 32], [16, 8], 0, 0, False)
    assert list(a.items()) == list(b.items()) and not any(k.startswith("contact_ae") for k in a)
    c = ot.teacher_param_shapes(15, 64, 6, [64, 32], [16, 8], 37, 5, False)
    assert c["actor_mlp.mlp.0.weight"] == (64, 15 + 8 + 5) and c["contact_ae.contact_dec_mlp.2.weight"] == (37, 32)
    o = ot.teacher_param_shapes(15, 64, 6, [64, 32], [16, 8], 37, 8, True)
    assert o["actor_mlp.mlp.0.weight"] == (64, 15 + 8)
