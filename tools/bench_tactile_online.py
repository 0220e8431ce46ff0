#!/usr/bin/env python
"""The online student's tactile augmentation in the distillation step, beside the gather it replaces and the torch ops it
stands for.

    python tools/bench_tactile_online.py [--rounds R] [--iters K] [--envs N] [--out profiles/tactile_online_augment.json]

(a) The tactile input of one minibatch: 8192 samples x 3 fingers of 32 x 64 out of the rollout storage's time-major arena of
    2048 envs x 32 steps (1.6 GB), three ways:
      gather : today's path, ``torch.ops.mi355ppo.gather_rows`` of the arena's rows -- no augmentation at all;
      fused  : ``TactileAugment.fused_seeded(arena2d, rows, seed)`` -- one CPU draw of the step's seed and ONE launch of
               k_tactile_augment_seeded, reading the arena in place;
      torch  : ``arena.index_select(0, rows)`` + ``TactileAugment.draw`` on the CPU (one row of parameters per image) +
               ``TactileAugment.apply`` in torch ops -- what calling the offline transform from the step would cost.
    Noise 0.001 and patch masking 0.3 at patch 16 in both augmenting paths.  The comparator of ``fused`` is ``torch``.
(b) One ``ExtrinsicAdapt.update_step`` + optimizer step, tactile + proprioception, 2048 envs x 32 steps, minibatch 8192
    (the configs[2] share), ``offline_train.tactile_augment_online`` "off" against "fused" in the same build.
Host clock around K iterations ending in a device synchronise, R alternating rounds in one job, medians with min .. max, in
ms per iteration.  The record is stamped with the library's build hash."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HORIZON, FINGERS, HW, MINI_EPOCHS = 32, 3, (32, 64), 8
NOISE, MASKING, PATCH = 0.001, 0.3, 16


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _rounds(paths, rounds, iters, warm):
    import torch
    for fn in paths.values():
        for i in range(warm):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                fn(i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / iters)
    return ms


def _summary(ms, a, b):
    med = {k: _median(v) for k, v in ms.items()}
    return {"ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            f"{a}_over_{b}": round(med[a] / med[b], 4),
            f"rounds_where_{a}_is_slower": [r for r in range(len(ms[a])) if ms[a][r] > ms[b][r]]}


def _engine(key, envs):
    """The workload of tools/bench_student.py --config 3 (same synthetic StudentBuffer, same O(1)-scale student)."""
    import torch
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=envs, horizon_length=HORIZON, rl_device="cuda:0", mini_epochs=MINI_EPOCHS, obs_info=True,
                         tactile_info=True, pcl_info=False, img_info=False, seg_info=False, num_points=8)
    cfg.offline_train.tactile_augment_online = key
    torch.manual_seed(0)
    env = SyntheticInsertionEnv(envs, device="cuda:0", tactile_hw=HW, pcl_points=0, img_hw=None)
    agent = ExtrinsicAdapt(env, None, cfg)
    g = torch.Generator(device="cuda:0").manual_seed(0)
    st = agent.storage.storage_dict
    st["n_tactile"].uniform_(0, 1, generator=g)
    st["n_student_obs"].normal_(generator=g)
    st["teacher_actions"].uniform_(-1.2, 1.2, generator=g)
    with torch.no_grad():
        for m in agent.student.model.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.kaiming_uniform_(m.weight, a=5 ** 0.5)
    agent.storage.prepare_training()
    agent.set_student_train()
    return agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tactile_online_augment.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tactile_online: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.models.transformer.utils import TactileAugment
    dev = "cuda:0"
    envs = args.envs
    n_rows, mb = envs * HORIZON, envs * HORIZON // MINI_EPOCHS
    # (a) the minibatch's tactile input
    g = torch.Generator(device=dev).manual_seed(0)
    arena2d = torch.rand(n_rows, FINGERS * HW[0] * HW[1], device=dev, generator=g)
    arena6d = arena2d.reshape(n_rows, 1, FINGERS, 1, *HW)
    perm = torch.randperm(n_rows, device=dev, generator=g)
    rows = [perm[k * mb:(k + 1) * mb].contiguous() for k in range(MINI_EPOCHS)]
    aug = TactileAugment(HW, HW, PATCH, NOISE, MASKING)
    seeds, draws = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)

    def gather(i):
        return torch.ops.mi355ppo.gather_rows([arena2d], rows[i % MINI_EPOCHS])[0]

    def fused(i):
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=seeds))
        return aug.fused_seeded(arena2d, rows[i % MINI_EPOCHS], seed)[0]

    def torch_path(i):
        x = arena6d.index_select(0, rows[i % MINI_EPOCHS])
        offsets, jitter, angles, keep, seed = aug.draw(mb * FINGERS, draws)
        return aug.apply(x, offsets, jitter, angles, keep, NOISE, seed)

    ms = _rounds({"gather": gather, "fused": fused, "torch": torch_path}, args.rounds, args.iters, 10)
    image_bytes = mb * FINGERS * HW[0] * HW[1] * 4
    part_a = {"config": f"{mb} samples x {FINGERS} fingers x {HW[0]} x {HW[1]} out of {n_rows} rows; noise {NOISE}, masking "
                        f"{MASKING} at patch {PATCH}", "bytes_read_plus_written": 2 * image_bytes,
              **_summary(ms, "fused", "torch")}
    med = part_a["ms_median"]
    part_a["fused_over_gather"] = round(med["fused"] / med["gather"], 4)
    part_a["fused_gb_per_s_host_clock"] = round(2 * image_bytes / (med["fused"] * 1e-3) / 1e9, 1)
    part_a["gather_gb_per_s_host_clock"] = round(2 * image_bytes / (med["gather"] * 1e-3) / 1e9, 1)
    del arena2d, arena6d
    # (b) one update_step + optimizer step, key off against key on
    agents = {k: _engine(k, envs) for k in ("off", "fused")}

    def step(agent):
        def run(i):
            agent.update_step(i % len(agent.storage))
            agent.optim.step(1.0)
        return run

    ms = _rounds({k: step(a) for k, a in agents.items()}, args.rounds, args.iters, 10)
    part_b = {"config": f"ExtrinsicAdapt.update_step + optimizer step, tactile + proprioception, {envs} envs x {HORIZON} steps, "
                        f"minibatch {mb}; the stock strengths (noise 0.001, no masking)", **_summary(ms, "fused", "off")}
    rec = {
        "tool": "tools/bench_tactile_online.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "method": f"host clock around {args.iters} iterations ending in a device synchronise (the CPU draws of both augmenting "
                  f"paths included); {args.rounds} alternating rounds in one job; ms per iteration",
        "kernel_time": "not measured by this tool (host clock only)",
        "minibatch_input": part_a,
        "update_step": part_b,
    }
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
