#!/usr/bin/env python
"""What KL early stopping costs to carry, and what a stopped update saves: the teacher update in one process.

    python tools/bench_kl_stop.py [--pairs R] [--updates K] [--out profiles/kl_early_stop_cost.json]
                                  [--parent-runs a,b,..] [--tree-runs a,b,..]

BASELINE configs[1] (4096 envs x 32 horizon, 8 x 8 optimizer steps per update).  Engines are built once on the same
problem and the same workspace allocation and warmed up.

(a) carrying the feature: an engine with kl_early_stop and a threshold nothing reaches against an engine without the
    switch, R alternating pairs of K whole updates (prepare + update, device synchronise around every round), ms per
    update.  The switched-on update pays the estimator's store and decision in the statistics block, one word read per
    gated kernel, and one host wait per mini-epoch (the look-ahead read of the stop word).  Target: within 1 % of the
    switched-off median.  --parent-runs / --tree-runs: updates/s of `bench.py --gpus 1 --steps 30 --warmup 5` (flagship
    section alone) on the parent
    commit's build and on this tree (switch off), alternated by the caller in the same job; recorded beside the pairs
    with the verdict whether each median lies inside the other's spread.  Target: within 1 % of the parent.
(b) what a stop saves: ms per update when the stop falls in mini-epoch 1, 4 and 7, against the full update.  Every timed
    update starts from the same snapshot (parameters, moments, normalisers), so it stops at the same step; the
    threshold of each row is the geometric mean of the estimator of two neighbouring steps of the snapshot's own
    sequence; the estimator is not monotone, so a stop may fall in an earlier mini-epoch than the one aimed at -- the
    row records where it fell.  Expectation: the stopping mini-epoch m plus one more of look-ahead, (m + 2) / 8 of the full
    update.  No bar.

The record is stamped with the library's build hash.
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
UNREACHABLE = 1e9
SNAP = ("params", "adam_m", "adam_v", "rms_obs", "rms_priv", "rms_value")


def _engine(stop, init, ro, perm, thr):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    eng = TeacherEngine(N, T, E, units=UNITS, priv_units=PRIV_UNITS, perm=perm, kl_early_stop=stop, kl_threshold=thr)
    eng.load_params(init)
    eng.prepare(ro)
    return eng


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _floats(text):
    return [float(x) for x in text.split(",") if x.strip()] if text else []


def _launches(eng):
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
    return sum(c["launches"] for c in classes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_early_stop_cost.json"))
    ap.add_argument("--parent-runs", default="")
    ap.add_argument("--tree-runs", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kl_stop: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from oracle import synth
    init, ro, perm = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, seed=1234)
    ro = {k: v.cuda() for k, v in ro.items()}
    engines = {"off": _engine(False, init, ro, perm, 0.008), "on": _engine(True, init, ro, perm, UNREACHABLE)}
    # ONE workspace allocation for both: the env level's time depends on the allocation it runs on (up to 2 % of the
    # update, TeacherEngine.tune_workspace), and the workspace holds nothing that outlives an update
    engines["on"].workspace = engines["off"].workspace
    n_mb = engines["on"].n_mb
    snap = {k: getattr(engines["on"], k).clone() for k in SNAP}

    def restore(eng):
        for k in SNAP:
            getattr(eng, k).copy_(snap[k])
        eng.adam_t = 0

    # ---- (a): the switch carried, nothing stops
    for eng in engines.values():           # warm-up: code loading, clocks
        for _ in range(3):
            eng.prepare()
            eng.update()
    torch.cuda.synchronize()
    assert engines["on"].stop_step is None
    ms = {"off": [], "on": []}
    for _ in range(args.pairs):
        for name in ("off", "on"):
            eng = engines[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                eng.prepare()
                eng.update()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.updates)
    assert engines["on"].stop_step is None
    med = {k: _median(v) for k, v in ms.items()}
    ratio = med["on"] / med["off"]

    # ---- (b): the snapshot's own estimator sequence, then a stop in mini-epochs 1, 4, 7
    on = engines["on"]
    restore(on)
    on.prepare()
    on.update()
    seq = on.approx_kl().double().numpy()
    rows = {}
    plan = [("full", None)] + [(f"mini_epoch_{m}", m) for m in (1, 4, 7)]
    thr_of = {}
    for name, m in plan:
        if m is None:
            thr_of[name] = UNREACHABLE
        else:
            k = m * n_mb + n_mb // 2                   # the stop step aimed at: the middle of mini-epoch m
            thr_of[name] = float((seq[k - 1] * seq[k]) ** 0.5) / 1.5
    times = {name: [] for name, _ in plan}
    stops = {}
    for _ in range(args.pairs):
        for name, m in plan:
            on.kl_threshold = thr_of[name]
            for _ in range(args.updates):
                restore(on)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                on.prepare()
                on.update()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
            stops[name] = on.stop_step
    full_ms = _median(times["full"])
    for name, m in plan:
        med_ms = _median(times[name])
        rows[name] = {"kl_threshold": thr_of[name], "stop_step": stops[name],
                      "stop_mini_epoch": None if stops[name] is None else stops[name] // n_mb,
                      "update_ms_median": round(med_ms, 4), "update_ms_min": round(min(times[name]), 4),
                      "update_ms_max": round(max(times[name]), 4), "over_full": round(med_ms / full_ms, 4),
                      "aimed_mini_epoch": m,     # the estimator is not monotone: the stop may fall earlier than aimed
                      "expected_over_full": None if stops[name] is None else round(min(stops[name] // n_mb + 2, E) / E, 4)}
    launches = {}
    for name, m in plan:
        on.kl_threshold = thr_of[name]
        restore(on)
        launches[name] = _launches(on)
    restore(engines["off"])
    launches["switch_off"] = _launches(engines["off"])

    rec = {
        "tool": "tools/bench_kl_stop.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "config": f"teacher PPO update {N} envs x {T} horizon, {E}x{n_mb} optimizer steps; {args.pairs} alternating "
                  f"rounds of {args.updates} updates",
        "a_carrying_the_switch": {
            "update_ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "update_ms_median": {k: round(v, 4) for k, v in med.items()},
            "on_over_off": round(ratio, 5),
            "target": "switch on with an unreachable threshold: median within 1 % of the switch-off median",
            "within_1_percent": bool(abs(ratio - 1.0) <= 0.01),
        },
        "b_stopped_updates": {
            "note": "every timed update restarts from one snapshot; prepare + update, one host synchronise behind it",
            "estimator_of_the_snapshot": [float(x) for x in seq],
            "rows": rows,
            "launches_per_update": launches,
        },
    }
    parent, tree = _floats(args.parent_runs), _floats(args.tree_runs)
    if parent and tree:
        mp_, mt = _median(parent), _median(tree)
        rec["a_carrying_the_switch"]["switch_off_vs_parent_commit"] = {
            "command": "bench.py --gpus 1 --steps 30 --warmup 5 (the flagship section alone: --no-cpu-baseline --no-roofline "
                       "--no-peak-probe --no-student --no-experiments --no-multi-configs), alternating parent build / "
                       "this tree in one job",
            "parent_updates_per_s": parent, "tree_updates_per_s": tree,
            "parent_median": mp_, "tree_median": mt, "tree_over_parent": round(mt / mp_, 5),
            "within_1_percent": bool(abs(mt / mp_ - 1.0) <= 0.01),
            "tree_median_inside_parent_spread": bool(min(parent) <= mt <= max(parent)),
            "parent_median_inside_tree_spread": bool(min(tree) <= mp_ <= max(tree)),
        }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
