"""KL early stopping under data parallelism (modelled on test_gpu_lr_schedule_dp.py): the library's own RCCL path on a
one-rank communicator must reproduce the single-GPU stopped update bit for bit, and two real processes on one GPU over
gloo, with different rollouts, must stop at the same step -- the decision taken from the rank mean of their estimators --
and hold equal parameters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kl_stop_cases as K
from tests import lr_schedule_cases as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["C", "adaptive"])
def test_native_rccl_update_on_a_one_rank_communicator_equals_the_single_gpu_stop(name):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from isaacgyminsertion_amd.utils.dist import NativeComm
    K.assert_margins(name)
    c = K.CASES[name]
    N, T, E = c["shape"]
    init, ro, perm = K.case_problem(name)
    torch.cuda.set_device(0)
    comm = NativeComm(rank=0, world=1)
    keys = ("params", "adam_m", "adam_v", "rms_obs", "rms_priv", "mus_w", "sigmas_w") + (("lr_state",) if c.get("adaptive") else ())

    def run(mode):
        eng = TeacherEngine(N, T, E, units=c["units"], priv_units=c["priv_units"], perm=perm, device="cuda:0",
                            obs_dim=L.OBS, lr=c["lr"], kl_early_stop=True, kl_threshold=c["thr"],
                            lr_schedule="adaptive" if c.get("adaptive") else "fixed")
        eng.load_params(init)
        eng.prepare(ro)
        if mode == "single":
            eng.update()
        else:
            eng.update_dp_native(comm, overlap=(mode == "overlap"))
        torch.cuda.synchronize()
        s = eng.stop_step
        assert s == c["stop"] and eng.adam_t == s
        out = {k: getattr(eng, k).clone() for k in keys}
        if "lr_state" in out:       # the exchange scratch (lr_state[1]) is only written by the data-parallel paths
            out["lr_state"] = torch.cat([out["lr_state"][:1], out["lr_state"][2:]])
        out["stats"] = eng.stats[:s].clone()
        out["row_s"] = eng.stats[s, :5].clone()
        out["approx_kl"] = eng.approx_kl()
        return out

    ref = run("single")
    for mode in ("overlap", "serial"):
        got = run(mode)
        for k in ref:
            assert torch.equal(ref[k], got[k]), (mode, k)
    comm.close()


def test_two_ranks_stop_at_the_same_step_from_the_rank_mean_estimator():
    env = dict(os.environ, IGI_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kl_stop_dp_check.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, (out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads(lines[-1])
    thr, mb, ranks = res["kl_threshold"], res["mb"], res["ranks"]
    assert len(ranks) == 2
    limit = 1.5 * thr
    for mode in ("serial", "overlapped"):
        a, b = ranks[0][mode], ranks[1][mode]
        s = a["stop"]
        print(mode, "stop", s, "rank-mean estimator", a["approx_kl"], "each rank alone", ranks[0]["alone"]["approx_kl"][:s + 1],
              ranks[1]["alone"]["approx_kl"][:s + 1])
        assert s is not None and 0 < s < 9 and b["stop"] == s                 # the same step, part of the way
        assert a["adam_t"] == b["adam_t"] == s
        assert a["approx_kl"] == b["approx_kl"] and len(a["approx_kl"]) == s + 1   # the same record, bit for bit
        assert a["params_sum"] == b["params_sum"]                           # parameters equal across ranks
        rec = np.array(a["approx_kl"])
        assert np.all(rec[:s] <= limit) and rec[s] > limit                    # the rule, on the mean
        assert a["rms_count"] == b["rms_count"] == 1 + (s + 1) * mb           # step s's minibatch ingested, nothing later
        # step 0 precedes every parameter change: there the mean is that of the two ranks' own first estimators
        alone0 = 0.5 * (np.float32(ranks[0]["alone"]["approx_kl"][0]) + np.float32(ranks[1]["alone"]["approx_kl"][0]))
        np.testing.assert_allclose(rec[0], alone0, rtol=1e-6)
    assert ranks[0]["serial"]["approx_kl"] == ranks[0]["overlapped"]["approx_kl"]
    assert ranks[0]["serial"]["params_sum"] == ranks[0]["overlapped"]["params_sum"]
