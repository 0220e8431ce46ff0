"""bench.py's plain run and --dump-outputs: a plain run carries the headline only, and the arrays it dumps are what the
last timed update computed -- the same arrays an engine fed the same seeded problem holds after warm-up + timed updates
(tune_workspace leaves the state bit for bit as it was, test_gpu_teacher.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, STEPS, WARMUP = 512, 32, 2, 1   # a shape test_gpu_teacher.py runs at 8 mini-epochs


def _engine(bench, dev):
    from isaacgyminsertion_amd.envs import synthetic_rollout as synth
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    init, ro, perm = synth.teacher_problem(N, T, bench.UNITS, bench.PRIV_UNITS, seed=1234, device=dev)
    eng = TeacherEngine(N, T, bench.MINI_EPOCHS, units=bench.UNITS, priv_units=bench.PRIV_UNITS, perm=perm, device=dev)
    eng.load_params(init)
    eng.set_rollout(ro)
    return eng


def test_bench_options():
    """--full and --dump-outputs exist; --steps below 1 is refused before anything starts"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout, out.stderr[-2000:]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_update(tmp_path):
    out_dir = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", str(WARMUP), "--envs", str(N), "--horizon", str(T), "--dump-outputs", str(out_dir)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    rec = json.loads(lines[0])
    assert rec["steps"] == STEPS and rec["warmup"] == WARMUP and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "updates/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["finite"]
    # nothing outside the headline ran
    assert rec["roofline"] is None and rec["cpu_baseline"] is None
    assert "student" not in rec and "experiments" not in rec and "kernels" not in rec

    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert {"stats", "params", "mus", "sigmas", "returns_raw"} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6

    import bench
    eng = _engine(bench, torch.device("cuda", 0))
    for _ in range(WARMUP + STEPS):
        eng.prepare()
        eng.update()
    torch.cuda.synchronize()
    ref_dir = tmp_path / "ref"
    bench.dump_outputs(str(ref_dir), eng)
    assert sorted(got) == sorted(f[:-4] for f in os.listdir(ref_dir))
    for k, a in got.items():
        np.testing.assert_array_equal(a, np.load(ref_dir / f"{k}.npy"), err_msg=k)


@pytest.mark.gpu
def test_dump_outputs_samples_the_same_rows_within_its_budget(tmp_path, monkeypatch):
    import bench
    eng = _engine(bench, torch.device("cuda", 0))
    eng.prepare()
    eng.update()
    torch.cuda.synchronize()
    bench.dump_outputs(str(tmp_path / "all"), eng)
    full = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    per_sample = ("returns_raw", "advantages", "values_n", "returns_n", "mus", "sigmas")
    fixed = sum(a.nbytes for k, a in full.items() if k not in per_sample)
    row_bytes = sum(full[k].nbytes for k in per_sample) // (N * T)
    keep = 100
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", fixed + keep * row_bytes)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), eng)
    idx = torch.randperm(N * T, generator=torch.Generator().manual_seed(0))[:keep].sort().values.numpy()
    total = 0
    for k, a in full.items():
        s1, s2 = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        np.testing.assert_array_equal(s1, s2, err_msg=k)
        want = a.reshape(N * T, -1)[idx] if k in per_sample else a
        np.testing.assert_array_equal(s1, want, err_msg=k)
        total += s1.nbytes
    assert total <= fixed + keep * row_bytes
