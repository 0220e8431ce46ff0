#!/usr/bin/env python
"""What the device-side learning-rate schedule costs: the fixed and the adaptive teacher update in one process.

    python tools/bench_lr_schedule.py [--pairs R] [--updates K] [--out profiles/lr_schedule_cost.json]
                                      [--parent-runs a,b,..] [--tree-runs a,b,..]

BASELINE configs[1] (4096 envs x 32 horizon, 8 x 8 optimizer steps per update).  A fixed-schedule and an adaptive engine
are built once on the same problem and the same workspace allocation, warmed up, then timed in R alternating pairs of K whole updates (prepare + update,
device synchronise around every round), ms per update.  The adaptive engine's threshold (rl_games' default 0.008) is
large against the first updates' KL, so the rate moves -- the record of the last update and `rate_moved` are part of the
output --; the arithmetic per optimizer step is the same either way.
Target: adaptive median within 1 % of the fixed median of the same job (derived cost: eight one-wave launches at ~4 us
plus a double division per Adam block, ~0.04 ms of 25 ms).  The library's dispatch profiler gives the per-update launch
count and the tail kernels' own times for both.

--parent-runs / --tree-runs: updates/s of `bench.py --steps 30 --warmup 5` on the parent commit's build and on this
tree (fixed schedule), alternated by the caller in the same job; recorded beside the pairs with the verdict whether each
median lies inside the other's spread.  The record is stamped with the library's build hash.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T, E = 4096, 32, 8
UNITS, PRIV_UNITS = [512, 256, 128], [256, 128, 8]
TAILS = ("k_sumsq_stats", "k_adam_gather", "k_clip_adam", "k_lr_schedule")


def _engine(schedule, init, ro, perm, thr):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    eng = TeacherEngine(N, T, E, units=UNITS, priv_units=PRIV_UNITS, perm=perm, lr_schedule=schedule, kl_threshold=thr)
    eng.load_params(init)
    eng.prepare(ro)
    return eng


def _profile(eng):
    import torch
    from isaacgyminsertion_amd import _lib
    eng.prepare()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        eng.update()
        torch.cuda.synchronize()
        classes = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    tails = {c["name"]: dict(launches=c["launches"], total_ms=round(c["total_ms"], 4),
                             avg_us=round(1e3 * c["total_ms"] / max(c["launches"], 1), 3))
             for c in classes if c["name"] in TAILS and c["launches"]}
    return dict(launches_per_update=sum(c["launches"] for c in classes), tail_kernels=tails)


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _floats(text):
    return [float(x) for x in text.split(",") if x.strip()] if text else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--kl-threshold", type=float, default=0.008)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-runs", default="")
    ap.add_argument("--tree-runs", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lr_schedule: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from oracle import synth
    init, ro, perm = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, seed=1234)
    ro = {k: v.cuda() for k, v in ro.items()}
    engines = {name: _engine(name, init, ro, perm, args.kl_threshold) for name in ("fixed", "adaptive")}
    # ONE workspace allocation for both: the env level's time depends on the allocation it runs on (up to 2 % of the
    # update, TeacherEngine.tune_workspace), and the workspace holds nothing that outlives an update
    engines["adaptive"].workspace = engines["fixed"].workspace
    for eng in engines.values():           # warm-up: code loading, clocks
        for _ in range(3):
            eng.prepare()
            eng.update()
    torch.cuda.synchronize()
    ms = {"fixed": [], "adaptive": []}
    for _ in range(args.pairs):
        for name in ("fixed", "adaptive"):
            eng = engines[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                eng.prepare()
                eng.update()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.updates)
    ada = engines["adaptive"]
    hist = ada.lr_history()
    _profile(engines["fixed"])             # untimed: the first profiled update of a process creates the event pool
    moved = bool((ada.stats[:, 7].max() != ada.stats[:, 7].min()).item()) or ada.lr != 2.5e-4
    med = {k: _median(v) for k, v in ms.items()}
    ratio = med["adaptive"] / med["fixed"]
    rec = {
        "tool": "tools/bench_lr_schedule.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "config": f"teacher PPO update {N} envs x {T} horizon, {E}x{E} optimizer steps; {args.pairs} alternating pairs "
                  f"of {args.updates} updates; adaptive kl_threshold {args.kl_threshold}",
        "update_ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "update_ms_median": {k: round(v, 4) for k, v in med.items()},
        "adaptive_over_fixed": round(ratio, 5),
        "target": "adaptive median within 1 % of the fixed median",
        "within_1_percent": bool(abs(ratio - 1.0) <= 0.01),
        "rate_moved": moved,
        "adaptive_rate_now": ada.lr,
        "adaptive_last_record_kl_lr": [[float(a), float(b)] for a, b in hist.tolist()],
        "profiler": {name: _profile(engines[name]) for name in ("fixed", "adaptive")},
    }
    parent, tree = _floats(args.parent_runs), _floats(args.tree_runs)
    if parent and tree:
        mp_, mt = _median(parent), _median(tree)
        rec["fixed_vs_parent_commit"] = {
            "command": "bench.py --gpus 1 --steps 30 --warmup 5, alternating parent build / this tree in one job",
            "parent_updates_per_s": parent, "tree_updates_per_s": tree,
            "parent_median": mp_, "tree_median": mt,
            "tree_median_inside_parent_spread": bool(min(parent) <= mt <= max(parent)),
            "parent_median_inside_tree_spread": bool(min(tree) <= mp_ <= max(tree)),
        }
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
