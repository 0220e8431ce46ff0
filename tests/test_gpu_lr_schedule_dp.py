"""The adaptive learning-rate schedule under data parallelism (modelled on test_gpu_dp.py): the library's own RCCL path
on a one-rank communicator must reproduce the single-GPU update bit for bit, and two real processes on one GPU over
gloo, with different rollouts, must hold identical rate records -- the rule applied to the rank-mean of their KL."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lr_schedule_cases as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_rccl_update_under_the_schedule_on_a_one_rank_communicator():
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from isaacgyminsertion_amd.utils.dist import NativeComm
    (N, T, E), units, priv_units, lr0, thr, _ = L.CASES["C"]
    init, ro, perm = L.case_problem("C")
    torch.cuda.set_device(0)
    comm = NativeComm(rank=0, world=1)

    def run(mode):
        eng = TeacherEngine(N, T, E, units=units, priv_units=priv_units, perm=perm, device="cuda:0", lr=lr0,
                            lr_schedule="adaptive", kl_threshold=thr)
        eng.load_params(init)
        eng.prepare(ro)
        if mode == "single":
            eng.update()
        else:
            eng.update_dp_native(comm, overlap=(mode == "overlap"))
        torch.cuda.synchronize()
        return eng.params.clone(), eng.stats.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.lr_state.clone()

    ref = run("single")
    assert L.decisions(lr0, ref[4][2:].reshape(E, 2)[:, 1].tolist()) == L.EXPECTED["C"]
    for mode in ("overlap", "serial"):
        got = run(mode)
        for k, (a, b) in enumerate(zip(ref, got)):
            if k == 4:      # the exchange scratch (lr_state[1]) is only written by the data-parallel paths
                a, b = torch.cat([a[:1], a[2:]]), torch.cat([b[:1], b[2:]])
            assert torch.equal(a, b), (mode, k)
    comm.close()


def test_two_ranks_take_the_same_decisions_from_the_rank_mean_kl():
    env = dict(os.environ, IGI_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lr_schedule_dp_check.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, (out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads(lines[-1])
    lr0, thr, ranks = res["lr0"], res["kl_threshold"], res["ranks"]
    assert len(ranks) == 2
    for mode in ("serial", "overlapped"):
        rec = [np.array(r[mode]["record"]) for r in ranks]
        assert rec[0].tolist() == rec[1].tolist(), mode                    # identical records on both ranks
        assert ranks[0][mode]["lr"] == ranks[1][mode]["lr"] == rec[0][-1, 1]
        assert ranks[0][mode]["params_sum"] == ranks[1][mode]["params_sum"]
        # the rank-mean of the two ranks' per-epoch KL, gathered from both stats tensors
        mean_kl = (np.array(ranks[0][mode]["epoch_kl"]) + np.array(ranks[1][mode]["epoch_kl"])) / 2
        print(mode, "rank-mean KL", mean_kl, "compared", rec[0][:, 0], "rates", rec[0][:, 1])
        np.testing.assert_allclose(rec[0][:, 0], mean_kl, rtol=1e-5)
        lr, n_mb = lr0, len(ranks[0][mode]["slot7"]) // len(mean_kl)
        for e, kl in enumerate(mean_kl):
            assert L.boundary_distance(kl, thr) >= L.MARGIN, (e, kl, thr)  # the 10 % condition on the mean
            for r in ranks:
                assert r[mode]["slot7"][e * n_mb:(e + 1) * n_mb] == [float(np.float32(lr))] * n_mb
            lr = L.rule(lr, float(kl), thr)
            assert rec[0][e, 1] == lr, (mode, e)
        assert lr != lr0
    assert ranks[0]["serial"]["record"] == ranks[0]["overlapped"]["record"]
