#!/usr/bin/env python
"""The online student's camera-pair augmentation in the distillation step, beside the gathers it replaces and the torch ops
it stands for.

    python tools/bench_img_online.py [--rounds R] [--iters K] [--envs N] [--parent-root DIR] [--out profiles/img_online_augment.json]

(a) The camera input of one minibatch: 8192 samples x 2 tensors of 54 x 96 out of the rollout storage's two time-major arenas
    of 2048 envs x 32 steps (1.36 GB each), three ways:
      gather : today's path, ``torch.ops.mi355ppo.gather_rows`` of both arenas' rows -- no augmentation at all;
      fused  : ``SyncTransform.fused_seeded(img2d, seg2d, rows, seed)`` -- one CPU draw of the step's seed and ONE launch of
               k_image_pair_augment_seeded, reading the arenas in place;
      torch  : two ``index_select``s + ``SyncTransform.draw_seeded`` on the CPU + ``SyncTransform.apply_seeded`` in torch ops.
    Rotation 1 degree, noise 0.01 and patch masking 0.3 at patch 16 in both augmenting paths.  The comparator of ``fused`` is
    ``torch``.
(b) One ``ExtrinsicAdapt.update_step`` + optimizer step of the camera student (img + seg + proprioception), 2048 envs x 32
    steps, minibatch 8192 -- the largest of the benchmark's online sizes --, ``offline_train.img_augment_online`` "off"
    against "fused" in the same build, the strengths of (a).
(c) With ``--parent-root DIR`` (a built checkout of the parent commit): the key-off step of (b) in this build against the
    same step in that build, ONE worker process per build and round, alternating in the same job.
Host clock around K iterations ending in a device synchronise, R alternating rounds in one job, medians with min .. max, in
ms per iteration.  The record is stamped with the library's build hash."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if "--root" in sys.argv:                               # a worker of (c): the package of another checkout
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HORIZON, HW, MINI_EPOCHS = 32, (54, 96), 8
ROTATION, NOISE, MASKING, PATCH = 1.0, 0.01, 0.3, 16


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _time(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _rounds(paths, rounds, iters, warm):
    import torch
    for fn in paths.values():
        for i in range(warm):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for r in range(rounds):
        for k, fn in paths.items():
            ms[k].append(_time(fn, iters))
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.4f} ms" for k, v in ms.items()), file=sys.stderr, flush=True)
    return ms


def _summary(ms, a, b):
    med = {k: _median(v) for k, v in ms.items()}
    return {"ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            f"{a}_over_{b}": round(med[a] / med[b], 4),
            f"rounds_where_{a}_is_slower": [r for r in range(len(ms[a])) if ms[a][r] > ms[b][r]]}


def _engine(key, envs):
    """The camera student of tools/bench_student.py on a synthetic StudentBuffer; ``key`` None leaves the key out of the
    config (a checkout that does not know it)."""
    import torch
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=envs, horizon_length=HORIZON, rl_device="cuda:0", mini_epochs=MINI_EPOCHS, obs_info=True,
                         tactile_info=False, pcl_info=False, img_info=True, seg_info=True, num_points=8)
    off = cfg.offline_train
    off.img_rotation_deg, off.img_gaussian_noise, off.img_masking_prob, off.img_patch_size = ROTATION, NOISE, MASKING, PATCH
    if key is None:
        off.pop("img_augment_online", None)
    else:
        off.img_augment_online = key
    torch.manual_seed(0)
    env = SyntheticInsertionEnv(envs, device="cuda:0", tactile_hw=None, pcl_points=0, img_hw=HW)
    agent = ExtrinsicAdapt(env, None, cfg)
    g = torch.Generator(device="cuda:0").manual_seed(0)
    st = agent.storage.storage_dict
    st["n_img"].uniform_(0, 1, generator=g)
    st["n_seg"].uniform_(0, 3, generator=g)
    st["n_student_obs"].normal_(generator=g)
    st["teacher_actions"].uniform_(-1.2, 1.2, generator=g)
    with torch.no_grad():
        for m in agent.student.model.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.kaiming_uniform_(m.weight, a=5 ** 0.5)
    agent.storage.prepare_training()
    agent.set_student_train()
    return agent


def _step(agent):
    def run(i):
        agent.update_step(i % len(agent.storage))
        agent.optim.step(1.0)
    return run


def _worker(envs, iters):
    """One round of the key-off step in the checkout ``--root`` names: one JSON line."""
    from isaacgyminsertion_amd import _lib
    run = _step(_engine(None, envs))
    for i in range(10):
        run(i)
    print(json.dumps({"ms": _time(run, iters), "build": _lib.lib().igi_build_info().decode()}))


def _control(parent_root, envs, rounds, iters):
    ms, builds = {"this": [], "parent": []}, {}
    for _ in range(rounds):
        for name, root in (("this", HERE), ("parent", os.path.abspath(parent_root))):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--envs", str(envs),
                                  "--iters", str(iters)], check=True, capture_output=True, text=True, cwd=root).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            ms[name].append(rec["ms"])
            builds[name] = rec["build"]
            print(f"worker {name}: {rec['ms']:.4f} ms", file=sys.stderr, flush=True)
    return {"config": f"the key-off step of update_step in this build against the parent commit's build, {envs} envs x {HORIZON} "
                      f"steps; one worker process per build and round, alternating", "builds": builds,
            **_summary(ms, "this", "parent")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: a, b")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "img_online_augment.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_img_online: no HIP device (timings are taken on the GPU only)")
    if args.worker:
        return _worker(args.envs, args.iters)
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.models.transformer.utils import define_img_transforms
    dev = "cuda:0"
    envs, skip = args.envs, set(args.skip.split(","))
    n_rows, mb = envs * HORIZON, envs * HORIZON // MINI_EPOCHS
    rec = {
        "tool": "tools/bench_img_online.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "method": f"host clock around {args.iters} iterations ending in a device synchronise (the CPU draws of both augmenting "
                  f"paths included); {args.rounds} alternating rounds in one job; ms per iteration",
        "kernel_time": "not measured by this tool (host clock only)",
    }
    if "a" not in skip:                                # (a) the minibatch's camera input
        g = torch.Generator(device=dev).manual_seed(0)
        img2d = torch.rand(n_rows, HW[0] * HW[1], device=dev, generator=g)
        seg2d = torch.rand(n_rows, HW[0] * HW[1], device=dev, generator=g)
        perm = torch.randperm(n_rows, device=dev, generator=g)
        rows = [perm[k * mb:(k + 1) * mb].contiguous() for k in range(MINI_EPOCHS)]
        aug = define_img_transforms(*HW, *HW, PATCH, NOISE, MASKING, ROTATION)[3]
        seeds, seeds_t = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)

        def gather(i):
            return torch.ops.mi355ppo.gather_rows([img2d, seg2d], rows[i % MINI_EPOCHS])

        def fused(i):
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=seeds))
            return aug.fused_seeded(img2d, seg2d, rows[i % MINI_EPOCHS], seed)

        def torch_path(i):
            r = rows[i % MINI_EPOCHS]
            x = img2d.index_select(0, r).reshape(mb, 1, 1, *HW)
            y = seg2d.index_select(0, r).reshape(mb, 1, 1, *HW)
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=seeds_t))
            offsets, angles, keep, seed = aug.draw_seeded(mb, 1, seed)
            return aug.apply_seeded(x, y, offsets, angles, keep, NOISE, seed)

        ms = _rounds({"gather": gather, "fused": fused, "torch": torch_path}, args.rounds, args.iters, 10)
        image_bytes = mb * 2 * HW[0] * HW[1] * 4
        part = {"config": f"{mb} samples x 2 tensors x {HW[0]} x {HW[1]} out of {n_rows} rows; rotation {ROTATION} degree, noise "
                          f"{NOISE}, masking {MASKING} at patch {PATCH}", "bytes_read_plus_written": 2 * image_bytes,
                **_summary(ms, "fused", "torch")}
        med = part["ms_median"]
        part["fused_over_gather"] = round(med["fused"] / med["gather"], 4)
        part["fused_gb_per_s_host_clock"] = round(2 * image_bytes / (med["fused"] * 1e-3) / 1e9, 1)
        part["gather_gb_per_s_host_clock"] = round(2 * image_bytes / (med["gather"] * 1e-3) / 1e9, 1)
        rec["minibatch_input"] = part
        del img2d, seg2d
    else:
        rec["minibatch_input"] = "not measured in this run"
    if "b" not in skip:                                # (b) one update_step + optimizer step, key off against key on
        agents = {k: _engine(k, envs) for k in ("off", "fused")}
        ms = _rounds({k: _step(a) for k, a in agents.items()}, args.rounds, args.iters, 10)
        rec["update_step"] = {"config": f"ExtrinsicAdapt.update_step + optimizer step, img + seg + proprioception, {envs} envs x "
                                        f"{HORIZON} steps, minibatch {mb}; rotation {ROTATION} degree, noise {NOISE}, masking "
                                        f"{MASKING} at patch {PATCH}", **_summary(ms, "fused", "off")}
        del agents
    else:
        rec["update_step"] = "not measured in this run"
    if args.parent_root:                               # (c) the key-off step against the parent commit's build
        torch.cuda.empty_cache()
        rec["key_off_against_parent"] = _control(args.parent_root, envs, args.rounds, args.iters)
    else:
        rec["key_off_against_parent"] = "not measured in this run (no --parent-root)"
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
