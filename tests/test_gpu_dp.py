"""Data-parallel paths on ONE GPU (the pool has single-GPU boxes; the driver runs the real N-GPU RCCL bench):

* the student's gradient exchange against the reference's own two-process run (tests/golden/student_dp2.npz,
  ext_adapt.py:833-851 under gloo): two 'ranks' are emulated in one process, their flat gradients summed (what
  all-reduce(SUM) produces) and applied with grad_scale = 1/2;
* two REAL processes, both on cuda:0, a real torch.distributed group (gloo carries device tensors): the teacher's
  one-call data-parallel update (igi_teacher_update_dp with async collectives issued from its callback) equals the
  serial schedule bit for bit on every rank, parameters are identical across ranks afterwards, and whole
  PPO.train() / ExtrinsicAdapt.train() jobs with multi_gpu=True end with identical parameters on both ranks.
  (teacher two-rank golden: test_gpu_teacher.py::test_dp_split_step_matches_reference_two_rank_golden)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "student_dp2.npz"))


def test_student_dp_matches_reference_two_rank_golden():
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    N, T, E = [int(x) for x in G["meta"]]
    agents = []
    for r in range(2):
        cfg = default_config(num_envs=N, horizon_length=T, rl_device="cuda:0", mini_epochs=E, obs_info=True,
                             pcl_info=True, num_points=8)
        cfg.offline_train.only_bc = True
        env = SyntheticInsertionEnv(N, device="cuda:0", pcl_points=800)
        a = ExtrinsicAdapt(env, None, cfg)
        a.student.model.load_state_dict({k[5:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("init/")})
        for k in a.storage.storage_dict:
            a.storage.storage_dict[k].copy_(torch.from_numpy(G[f"r{r}/in/{k}"]))
        a.storage.indices.copy_(torch.from_numpy(G[f"r{r}/perm"]))
        a.storage.prepare_training()
        a.set_student_train()
        agents.append(a)
    losses = [[], []]
    for _ in range(E):
        for i in range(len(agents[0].storage)):
            for r, a in enumerate(agents):
                la, _ = a.update_step(i)
                losses[r].append(la)
            total = agents[0].optim.flat_grad + agents[1].optim.flat_grad      # all-reduce(SUM)
            for a in agents:
                a.optim.flat_grad.copy_(total)
                a.optim.step(0.5)                                              # / rank_size folded into clip + Adam
    torch.cuda.synchronize()
    assert torch.equal(agents[0].optim.flat, agents[1].optim.flat)             # ranks stay identical
    k = len(losses[0])
    for r in range(2):
        np.testing.assert_allclose(torch.stack(losses[r]).cpu().numpy(), G[f"r{r}/action_losses"], rtol=2e-4)
    for name, v in agents[0].student.model.state_dict().items():
        ref = G[f"final/{name}"]
        np.testing.assert_allclose(v.cpu().numpy(), ref, atol=k * 3e-4 * 0.25, err_msg=name)
        assert np.abs(v.cpu().numpy() - ref).mean() <= k * 3e-4 * 0.03, name


def test_two_process_data_parallel_on_one_gpu():
    env = dict(os.environ, IGI_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dp_2proc_check.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=900)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, (out.stdout[-2000:], out.stderr[-3000:])
    res = json.loads(lines[-1])
    assert res["ok"] and res["overlapped_equals_serial"] and res["params_identical_across_ranks"]
    assert res["ppo_train_multi_gpu_params_identical"] and res["ext_adapt_train_multi_gpu_params_identical"]
    assert res["one_call_update_dp_equals_stepwise"]
    assert res["student_two_bucket_exchange_equals_serial"]   # FlatAdam's early bucket against real two-rank reductions


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 2` started as ONE process, the way the driver starts every bench: the parent must start
    the two ranks itself (torchrun as a child, scripts/train_s1.sh:16 in the reference), rank 0's single JSON line must
    come through with n_gpus == 2, identical parameters on both ranks, and every multi-GPU sub-record free of errors.
    Both ranks share cuda:0 here and the gradients travel over gloo (IGI_DIST_BACKEND); the exchange semantics are the
    reference's (frozen_ppo.py:586-603, ext_adapt.py:833-851)."""
    env = dict(os.environ, IGI_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--full", "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    # TWO lines at N > 1 (round 6): the complete headline record FIRST, before the multi-GPU sub-records start (a hang in a
    # sub-record cannot cost the headline), then the same record extended by multi_gpu_configs
    assert out.returncode == 0 and len(lines) == 2, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    head, res = json.loads(lines[0]), json.loads(lines[1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert head[k] == res[k], k
    assert isinstance(head["multi_gpu_configs"], str)
    assert res["n_gpus"] == 2 and res["finite"] and res["params_identical_across_ranks"]
    assert res["value"] > 0 and res["config"]["parallelism"] == "dp2"
    assert "rccl_ranks" in res["config"]         # None here (gloo carries the gradients); ncclCommCount under RCCL
    assert res["roofline"] is not None           # the instrumented region ran the data-parallel step on both ranks
    assert res["roofline"]["peak_measured_mfma"] > 50 and 1.0 < res["roofline"]["peak_measured_clock_ghz"] < 2.6
    multi = res["multi_gpu_configs"]
    recs = {k: v for k, v in multi.items() if k != "note"}
    assert len(recs) >= 6, list(recs)
    for name, rec in recs.items():
        assert "error" not in rec and "skipped" not in rec, (name, rec)
        subs = [v for v in rec.values() if isinstance(v, dict)]
        flat = subs if subs and all(isinstance(v, (dict, float, int)) for v in rec.values()) and "tflops" not in rec else [rec]
        for r in flat:
            assert r.get("params_identical_across_ranks", True) is True, (name, r)
            # a per-GPU fraction of the peak is a fraction (round 5 multiplied the flops by the world size and divided by
            # ONE GPU's peak: 6 - 7 on eight GPUs)
            if "frac_of_f32_mfma_peak" in r:
                assert 0 < r["frac_of_f32_mfma_peak"] <= 1.0, (name, r)


def test_bench_parent_fails_when_a_rank_fails():
    """a failed child must turn into a non-zero exit code of the parent (no JSON line, no hang)"""
    env = dict(os.environ, IGI_DIST_BACKEND="no-such-backend", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--no-cpu-baseline", "--no-roofline", "--no-multi-configs"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_native_rccl_update_on_a_one_rank_communicator():
    """The library's own RCCL path (csrc/comm.h: ncclCommInitRank, the communication stream, the event fences, the
    grouped bucket all-reduces, the stats all-reduce) on a ONE-rank communicator on cuda:0 -- every RCCL call of the
    data-parallel update executes; with one rank a SUM all-reduce is the identity and 1/world = 1, so the overlapped
    and the serial native schedules must both reproduce igi_teacher_update bit for bit (parameters, per-step
    statistics, Adam moments), and stats_sum == stats."""
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from isaacgyminsertion_amd.utils.dist import NativeComm
    from oracle import synth
    N, T, E = 512, 8, 4
    units, priv = [512, 256, 128], [256, 128, 8]
    init, ro, perm = synth.teacher_problem(N, T, units, priv, seed=21, done_p=0.05)
    torch.cuda.set_device(0)
    comm = NativeComm(rank=0, world=1)
    assert comm.handle and comm.world == 1
    # what RCCL itself reports (ncclCommCount / ncclGetVersion): the figure bench.py puts in config.rccl_ranks
    assert comm.rccl_ranks() == 1 and comm.rccl_version().count(".") == 2
    t = torch.arange(1000, dtype=torch.float32, device="cuda:0")
    assert torch.equal(comm.all_reduce_(t.clone()), t) and torch.equal(comm.broadcast_(t.clone()), t)

    def run(mode):
        eng = TeacherEngine(N, T, E, units=units, priv_units=priv, perm=perm, device="cuda:0")
        eng.load_params(init)
        eng.prepare(ro)
        ssum = None
        if mode == "single":
            eng.update()
        else:
            _, ssum = eng.update_dp_native(comm, overlap=(mode == "overlap"), want_stats_sum=True)
        torch.cuda.synchronize()
        return eng.params.clone(), eng.stats.clone(), eng.adam_m.clone(), eng.adam_v.clone(), ssum

    ref = run("single")
    for mode in ("overlap", "serial", "overlap"):
        got = run(mode)
        for a, b in zip(ref[:4], got[:4]):
            assert torch.equal(a, b), mode
        assert torch.equal(got[4], got[1]), mode
    assert torch.isfinite(ref[0]).all()
    comm.close()


def test_student_native_exchange_on_a_one_rank_communicator():
    """ExtrinsicAdapt.update() with the gradient exchange issued through the library's communicator (the decoder-side
    bucket handed over from INSIDE backward, on the communication stream, the encoders' bucket behind backward, clip +
    Adam behind igi_comm_join) on a ONE-rank communicator: every call of the overlapped schedule executes, a SUM over
    one rank is the identity and 1/world = 1, so the overlapped and the serial native schedules must reproduce the
    single-GPU update BIT FOR BIT -- losses and parameters (the student update is bitwise reproducible:
    test_gpu_student_scale.py::test_student_update_is_bitwise_reproducible)."""
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    from isaacgyminsertion_amd.utils.dist import NativeComm
    N, T, E = 64, 8, 4

    def make():
        cfg = default_config(num_envs=N, horizon_length=T, rl_device="cuda:0", mini_epochs=E, obs_info=True,
                             tactile_info=True, pcl_info=True, num_points=8)
        cfg.offline_train.only_bc = True
        env = SyntheticInsertionEnv(N, device="cuda:0", tactile_hw=(32, 64), pcl_points=800)
        torch.manual_seed(5)
        a = ExtrinsicAdapt(env, None, cfg)
        g = torch.Generator(device="cuda:0").manual_seed(3)
        st = a.storage.storage_dict
        st["n_tactile"].uniform_(0, 1, generator=g)
        st["n_student_obs"].normal_(generator=g)
        st["teacher_actions"].uniform_(-1.2, 1.2, generator=g)
        st["n_pcl"].normal_(0, 0.5, generator=g)
        with torch.no_grad():
            for m in a.student.model.modules():
                if isinstance(m, torch.nn.Linear):
                    torch.nn.init.kaiming_uniform_(m.weight, a=5 ** 0.5)
        a.storage.prepare_training()
        a.set_student_train()
        return a

    def run(mode):
        a = make()
        if mode != "single":
            a.multi_gpu, a.rank_size = True, 1
            a._comm = comm
        os.environ["IGI_DP_OVERLAP"] = "1" if mode == "overlap" else "0"
        try:
            losses, _ = a.update()
        finally:
            os.environ.pop("IGI_DP_OVERLAP", None)
        torch.cuda.synchronize()
        if mode == "overlap":   # the early bucket really left from inside backward (after the first, learning, step)
            assert a.optim._early_live and a.optim._early_done and a.optim.n_late > 0 and a.optim.late_floats > 0
        return torch.stack(losses).cpu(), a.optim.flat.detach().cpu().clone()

    torch.cuda.set_device(0)
    comm = NativeComm(rank=0, world=1)
    ref_l, ref_p = run("single")
    for mode in ("overlap", "serial", "overlap"):
        l, p = run(mode)
        assert torch.isfinite(p).all()
        assert torch.equal(l, ref_l) and torch.equal(p, ref_p), mode
    comm.close()
