#!/usr/bin/env python
"""The teacher with ground-truth contacts against the same teacher without them, in one process.

    python tools/bench_contacts.py [--rounds R] [--updates K] [--points P]

BASELINE configs[1] (4096 envs x 32 horizon, 8 x 8 optimizer steps per update) with P = 400 contact points and an
8-wide contact embedding.  Contact-on and contact-off engines are built once, warmed up, then timed in R alternating
rounds of K whole updates each (device synchronise around every round).  Also times model_act's forward at 4096 envs
(actor_critic_infer vs actor_critic_infer_contacts), counts the launches of one optimizer step with the library's
dispatch profiler, and prints one JSON line.
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


def _engine(contacts, P, init, ro, perm):
    import torch
    from isaacgyminsertion_amd.teacher_native import TeacherEngine, teacher_param_shapes
    kw = dict(contact_points=P, contact_emb=8) if contacts else {}
    eng = TeacherEngine(N, T, E, units=UNITS, priv_units=PRIV_UNITS, perm=perm, **kw)
    g = torch.Generator().manual_seed(7)
    params = {}
    for k, shp in teacher_param_shapes(15, 64, 6, UNITS, PRIV_UNITS, P if contacts else 0, 8 if contacts else 0).items():
        if k in init and tuple(init[k].shape) == tuple(shp):
            params[k] = init[k]
        else:
            params[k] = torch.randn(*shp, generator=g) / (shp[-1] ** 0.5) if len(shp) == 2 else torch.zeros(shp)
    eng.load_params(params)
    r = {k: v.cuda() for k, v in ro.items() if contacts or k != "contacts"}
    eng.prepare(r)
    return eng, r


def _launches_per_step(eng):
    import torch
    from isaacgyminsertion_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        eng.update()
        torch.cuda.synchronize()
        classes = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    return sum(c["launches"] for c in classes) / (E * E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--points", type=int, default=400)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_contacts: no HIP device (timings are taken on the GPU only)")
    from oracle import synth
    P = args.points
    init, ro, perm = synth.teacher_problem(N, T, UNITS, PRIV_UNITS, seed=1234)
    g = torch.Generator().manual_seed(11)
    ro = dict(ro)
    ro["contacts"] = (torch.rand(T, N, P, generator=g) < 0.1).float()
    engines = {name: _engine(name == "on", P, init, ro, perm) for name in ("off", "on")}
    for eng, _ in engines.values():        # warm-up: code loading, clocks
        eng.update()
        eng.update()
    torch.cuda.synchronize()
    ms = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            eng, r = engines[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                eng.prepare(r)
                eng.update()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.updates)
    launches = {name: _launches_per_step(engines[name][0]) for name in ("off", "on")}
    # model_act forward at 4096 envs
    obs = torch.randn(N, 15, device="cuda")
    priv = torch.randn(N, 64, device="cuda")
    cts = (torch.rand(N, P, device="cuda") < 0.1).float()
    act_us = {}
    for name in ("off", "on"):
        eng = engines[name][0]
        call = (lambda: eng.infer_contacts(obs, priv, cts, want_latent=True)) if name == "on" else \
            (lambda: eng.infer(obs, priv, want_latent=True))
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            call()
        torch.cuda.synchronize()
        act_us[name] = (time.perf_counter() - t0) * 1e6 / 200
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({
        "config": f"teacher PPO update {N} envs x {T} horizon, {E}x{E} optimizer steps, P = {P}, contact embedding 8",
        "update_ms_median": {k: round(v, 3) for k, v in med.items()},
        "update_ms_rounds": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "on_off_ratio": round(med["on"] / med["off"], 4),
        "launches_per_optimizer_step": launches,
        "model_act_us_4096": {k: round(v, 1) for k, v in act_us.items()},
    }))


if __name__ == "__main__":
    main()
