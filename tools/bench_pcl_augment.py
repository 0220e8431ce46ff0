#!/usr/bin/env python
"""The point-cloud augmentation of an environment step in one launch, beside the torch ops it replaces.

    python tools/bench_pcl_augment.py [--rounds R] [--iters K] [--out profiles/pcl_augment.json]

The cloud tensor of 4096 envs x (400 plug + 400 socket) points, fp32, in two configurations:
  noise only    : what the reference's ``augment`` applies today (PclProbNoise 0.7);
      torch : ``PointCloudAugmentations.augment`` as the reference's environment calls it (factory_task_insertion.py:
              951-986): plug and socket separately, each on the boolean-masked subset of the envs
              (``pts[mask] = augment(pts[mask], angle[mask], axes[mask], noise[mask])``);
  everything on : rotation 30 degrees, outliers 0.1, dropout 0.2;
      torch : the chain ``random_noise -> random_rotate -> add_outliers -> batch_random_dropout`` of the same class, called the
              same way;
  fused : ``PclAugment.fused(clouds, episode)`` -- one CPU draw of the step's seed and ONE launch of k_pcl_augment.
Host clock around K calls ending in a device synchronise, R alternating rounds, medians with min .. max, in ms per call.
Then the rollout: ``ExtrinsicAdapt.play_steps`` at 512 envs x 32 steps with ``task.env.pcl_augment`` off and "fused", ms per
rollout, R alternating rounds.  The record is stamped with the library's build hash.  No bar: the pairs are stated in README
as they come out."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_ENVS, POINTS = 4096, [400, 400]
CONFIGS = {"noise_only": dict(), "everything_on": dict(rot_deg=30.0, outlier_ratio=0.1, dropout_ratio=0.2)}


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


def _engine(key, n_envs, horizon):
    import torch
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=n_envs, horizon_length=horizon, rl_device="cuda:0", obs_info=True, pcl_info=True)
    cfg.task.env.pcl_augment = key
    torch.manual_seed(0)
    env = SyntheticInsertionEnv(n_envs, device="cuda:0", pcl_points=sum(POINTS))
    agent = ExtrinsicAdapt(env, None, cfg)
    agent.obs = env.reset()
    agent.set_student_eval()
    return agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rollouts", type=int, default=3, help="play_steps calls per round of the rollout measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcl_augment.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcl_augment: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.envs.pcl_augment import PclAugment, PointCloudAugmentations
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    clouds = (0.3 * torch.randn(N_ENVS, 1, 1, 3, generator=g) + 0.05 * torch.randn(N_ENVS, 1, sum(POINTS), 3, generator=g))
    clouds = clouds.reshape(N_ENVS, 1, -1).to(dev)
    episode = torch.zeros(N_ENVS, dtype=torch.int32, device=dev)
    angle = (torch.rand(N_ENVS, generator=g) * 2 - 1).to(dev) * (30.0 * math.pi / 180)
    axes = torch.randint(0, 3, (N_ENVS,), generator=g).to(dev)
    pos_noise = torch.randn(N_ENVS, 1, 3, generator=g).to(dev)
    ref = PointCloudAugmentations()
    results = {}
    for name, kw in CONFIGS.items():
        aug = PclAugment(POINTS, hit_prob=0.7, seed=1, **kw)

        def chain(pts, ang, ax, pn):
            if name == "noise_only":
                return ref.augment(pts, ang, ax, pn)
            pts = ref.random_noise(pts, pn)
            pts = ref.random_rotate(pts, ang, ax)
            pts = ref.add_outliers(pts)
            return ref.batch_random_dropout(pts)

        def fused(i):
            return aug.fused(clouds, episode)

        def torch_path(i):
            mask = torch.rand(N_ENVS, device=dev) > 1 - 0.7
            pts = clouds.reshape(N_ENVS, -1, 3)
            plug, socket = pts[:, :POINTS[0]].clone(), pts[:, POINTS[0]:].clone()
            plug[mask] = chain(plug[mask], angle[mask], axes[mask], pos_noise[mask])
            socket[mask] = chain(socket[mask], angle[mask], axes[mask], pos_noise[mask])
            return torch.cat([plug, socket], 1).reshape(clouds.shape)

        ms = _rounds({"fused": fused, "torch": torch_path}, args.rounds, args.iters, 20)
        results[name] = {"config": "hit_prob 0.7, " + (", ".join(f"{k} {v}" for k, v in kw.items()) or "noise only"),
                         "bytes_moved_per_call": 2 * N_ENVS * sum(POINTS) * 12, **_summary(ms, "fused", "torch")}
        gbs = results[name]["bytes_moved_per_call"] / (results[name]["ms_median"]["fused"] * 1e-3) / 1e9
        results[name]["fused_gb_per_s_host_clock"] = round(gbs, 1)
    del clouds
    n_envs, horizon = 512, 32
    agents = {"off": _engine("off", n_envs, horizon), "fused": _engine("fused", n_envs, horizon)}
    ms = _rounds({k: (lambda i, a=a: a.play_steps()) for k, a in agents.items()}, args.rounds, args.rollouts, 1)
    rollout = {"config": f"ExtrinsicAdapt.play_steps, {n_envs} envs x {horizon} steps, obs + point cloud (400 + 400 points), "
                         f"{args.rollouts} rollouts per round", **_summary(ms, "fused", "off")}
    rec = {
        "tool": "tools/bench_pcl_augment.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "shape": f"{N_ENVS} envs x ({POINTS[0]} + {POINTS[1]}) points; host clock around {args.iters} calls ending in a device "
                 f"synchronise (the CPU draw of the fused path and the mask draw of the torch path included); {args.rounds} "
                 f"alternating rounds",
        "kernel_time": "not measured by this tool (host clock only)",
        "configurations": results,
        "rollout": rollout,
    }
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
