#!/usr/bin/env python
"""The teacher with a shared actor-critic trunk (train.ppo.shared_parameters) against the separate critic, in one process.

    python tools/bench_shared_critic.py [--pairs R] [--updates K] [--out profiles/shared_critic.json]

BASELINE configs[1] (4096 envs x 32 horizon, 8 x 8 optimizer steps per update, default widths).  Both engines are built
once on the same rollout and permutation, warmed up, then timed in R >= 3 alternating pairs of K whole updates each
(device synchronise around every leg).  Then one update of each under the library's dispatch profiler (igi_prof_*):
launches per optimizer step and the per-class table.  Yardsticks: the same job's separate-critic figure, and the
algorithmic ratio 0.563 (6 x forward MACs x samples x mini-epochs: 2.531 -> 1.426 TFLOP per update); the record states the
shared update's fraction of the fp32-MFMA peak on its own FLOP count.  No target is set.  Writes the record (stamped with
the build hash) to --out and prints it as one JSON line."""
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
PEAK_F32_MFMA_TFLOPS = 157.3
FWD_MACS = {"separate": 402304, "shared": 226688}       # per sample, default widths (heads included)


def update_tflop(kind):
    """forward + data gradient + weight gradient = 3 x 2 x MACs, over N * T samples, E mini-epochs."""
    return 6.0 * FWD_MACS[kind] * N * T * E / 1e12


def _engine(shared, init, ro, perm):
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    eng = TeacherEngine(N, T, E, units=UNITS, priv_units=PRIV_UNITS, perm=perm, shared_parameters=shared)
    eng.load_params({k: v for k, v in init.items() if not (shared and k.startswith("critic_mlp"))})
    eng.prepare(ro)
    return eng


def _profile(eng, ro):
    import torch
    from isaacgyminsertion_amd import _lib
    eng.prepare(ro)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        eng.update()
        torch.cuda.synchronize()
        classes = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    table = {c["name"]: {"launches": c["launches"], "total_ms": round(c["total_ms"], 4)} for c in classes if c["launches"]}
    return sum(c["launches"] for c in classes) / (E * E), table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_critic.json"))
    args = ap.parse_args()
    if args.pairs < 3:
        raise SystemExit("bench_shared_critic: at least three alternating pairs")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_shared_critic: no HIP device (timings are taken on the GPU only)")
    import __graft_entry__ as ge
    from oracle import synth
    init, ro, perm = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, seed=1234)
    ro = {k: v.cuda() for k, v in ro.items()}
    engines = {"separate": _engine(False, init, ro, perm), "shared": _engine(True, init, ro, perm)}
    for eng in engines.values():           # warm-up: code loading, clocks
        eng.update()
        eng.update()
    torch.cuda.synchronize()
    ms = {k: [] for k in engines}
    for _ in range(args.pairs):
        for name, eng in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                eng.prepare(ro)
                eng.update()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.updates)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    prof = {k: _profile(eng, ro) for k, eng in engines.items()}
    rec = {
        "build": ge.library_hash(),
        "config": f"teacher PPO update {N} envs x {T} horizon, {E}x{E} optimizer steps, default widths; prepare + update",
        "update_ms_median": {k: round(v, 3) for k, v in med.items()},
        "update_ms_pairs": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "shared_over_separate": round(med["shared"] / med["separate"], 4),
        "shared_over_separate_pairs": [round(b / a, 4) for a, b in zip(ms["separate"], ms["shared"])],
        "algorithmic_ratio": round(FWD_MACS["shared"] / FWD_MACS["separate"], 4),
        "tflop_per_update": {k: round(update_tflop(k), 3) for k in engines},
        "frac_of_f32_mfma_peak": {k: round(update_tflop(k) / (med[k] * 1e-3) / PEAK_F32_MFMA_TFLOPS, 4) for k in engines},
        "launches_per_optimizer_step": {k: prof[k][0] for k in engines},
        "classes": {k: prof[k][1] for k in engines},
    }
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
