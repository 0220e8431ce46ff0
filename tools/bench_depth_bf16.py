#!/usr/bin/env python
"""The depth backbone's opt-in bf16-input mode (offline_train.model.depth_bf16_inputs / ops.depth_bf16_inputs) against the
fp32 path of the SAME build, and the fp32 path against the parent commit's build.

    python tools/bench_depth_bf16.py [--rounds R] [--seconds S] [--envs N] [--parent-root DIR] [--out profiles/depth_bf16.json]

(a) One ``DepthOnlyFCBackbone54x96`` (latent 32), forward + backward, at 8192 images.
(b) One ``ExtrinsicAdapt.update_step`` + optimizer step of the camera student (img + seg + proprioception), 2048 envs x 32
    steps, minibatch 8192: two backbones per step.
    Both with the switch off and on in one process, alternating, R rounds.
(c) With ``--parent-root DIR`` (a built checkout of the parent commit): (a) and (b) with the switch off in this build against
    the same in that build, ONE worker process per build and round, alternating in the same job.
Host clock around enough iterations to reach S seconds (counted once per path from a short probe), ending in a device
synchronise; medians with min .. max, in ms per iteration.  The per-class figures of one instrumented iteration of (a) per
mode (igi_prof_*: dispatch timestamps, the launch site's algorithmic FLOPs) go in beside them.  Stamped with the build hash."""
import argparse
import json
import math
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

HORIZON, HW, MINI_EPOCHS, IMAGES = 32, (54, 96), 8, 8192


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


def _iters_for(fn, seconds, warm=5):
    for i in range(warm):
        fn(i)
    return max(5, int(math.ceil(seconds * 1e3 / _time(fn, 5))))


def _rounds(paths, rounds, seconds):
    iters = {k: _iters_for(fn, seconds) for k, fn in paths.items()}
    ms = {k: [] for k in paths}
    for r in range(rounds):
        for k, fn in paths.items():
            ms[k].append(_time(fn, iters[k]))
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.4f} ms" for k, v in ms.items()), file=sys.stderr, flush=True)
    return ms, iters


def _summary(ms, a, b):
    med = {k: _median(v) for k, v in ms.items()}
    return {"ms_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            f"{a}_over_{b}": round(med[a] / med[b], 4),
            f"rounds_where_{a}_is_slower": [r for r in range(len(ms[a])) if ms[a][r] > ms[b][r]]}


def _switch(on):
    """igi_depth_set_bf16_inputs where the checkout has it (the parent commit's does not: off is all it knows)"""
    from isaacgyminsertion_amd import _lib
    fn = getattr(_lib.lib(), "igi_depth_set_bf16_inputs", None)
    if fn is None:
        assert not on
        return
    fn(1 if on else 0)


def _backbone(images=IMAGES):
    import torch
    from isaacgyminsertion_amd.algo.models.transformer.depth_backbone import DepthOnlyFCBackbone54x96
    torch.manual_seed(0)
    m = DepthOnlyFCBackbone54x96(latent_dim=32).cuda()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    x = torch.rand(images, 1, *HW, device="cuda:0", generator=g)
    gy = torch.randn(images, 32, device="cuda:0", generator=g)

    def run(on):
        def f(i):
            _switch(on)
            m.zero_grad(set_to_none=True)
            m(x).backward(gy)
            _switch(False)
        return f
    return run


def _engine(envs):
    """the camera student of tools/bench_img_online.py on a synthetic StudentBuffer, no augmentation, no mode key"""
    import torch
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=envs, horizon_length=HORIZON, rl_device="cuda:0", mini_epochs=MINI_EPOCHS, obs_info=True,
                         tactile_info=False, pcl_info=False, img_info=True, seg_info=True, num_points=8)
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

    def run(on):
        def f(i):
            _switch(on)            # the process switch: the config carries no key, so the Runner leaves it alone
            agent.update_step(i % len(agent.storage))
            agent.optim.step(1.0)
            _switch(False)
        return f
    return run


def _classes(fn):
    """per-class figures of one instrumented call"""
    import torch
    from isaacgyminsertion_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        fn(0)
        torch.cuda.synchronize()
        rows = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    return [{"name": k["name"], "launches": k["launches"], "us": round(1e3 * k["total_ms"], 1),
             "tflops": round(k["flops"] / max(k["total_ms"], 1e-9) / 1e9, 1)}
            for k in sorted(rows, key=lambda k: -k["total_ms"]) if k["name"].startswith("gemm_dma") or k["total_ms"] > 0.05]


def _worker(envs, seconds):
    """One round of (a) and (b) with the switch off in the checkout ``--root`` names: one JSON line."""
    import torch
    from isaacgyminsertion_amd import _lib
    a = _backbone()(False)
    ms_a = _time(a, _iters_for(a, seconds))
    del a
    torch.cuda.empty_cache()
    b = _engine(envs)(False)
    ms_b = _time(b, _iters_for(b, seconds))
    print(json.dumps({"backbone_ms": ms_a, "step_ms": ms_b, "build": _lib.lib().igi_build_info().decode()}))


def _control(parent_root, envs, rounds, seconds):
    ms = {"backbone": {"this": [], "parent": []}, "step": {"this": [], "parent": []}}
    builds = {}
    for _ in range(rounds):
        for name, root in (("this", HERE), ("parent", os.path.abspath(parent_root))):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--envs", str(envs),
                                  "--seconds", str(seconds)], check=True, capture_output=True, text=True, cwd=root).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            ms["backbone"][name].append(rec["backbone_ms"])
            ms["step"][name].append(rec["step_ms"])
            builds[name] = rec["build"]
            print(f"worker {name}: backbone {rec['backbone_ms']:.4f} ms, step {rec['step_ms']:.4f} ms", file=sys.stderr, flush=True)
    return {"config": "switch off in this build against the parent commit's build: (a) and (b) as above; one worker process "
                      "per build and round, alternating", "builds": builds,
            "backbone": _summary(ms["backbone"], "this", "parent"), "update_step": _summary(ms["step"], "this", "parent")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "depth_bf16.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_bf16: no HIP device (timings are taken on the GPU only)")
    if args.worker:
        return _worker(args.envs, args.seconds)
    from isaacgyminsertion_amd import _lib
    rec = {
        "tool": "tools/bench_depth_bf16.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "method": f"host clock around enough iterations to reach {args.seconds} s, ending in a device synchronise; "
                  f"{args.rounds} alternating rounds in one job; ms per iteration",
        "kernel_time": "profiler classes: dispatch timestamps of one instrumented iteration per mode (igi_prof_*), not rocprofv3",
    }
    bb = _backbone()
    paths = {"off": bb(False), "on": bb(True)}
    ms, iters = _rounds(paths, args.rounds, args.seconds)
    rec["backbone"] = {"config": f"DepthOnlyFCBackbone54x96(latent 32), forward + backward, {IMAGES} images", "iterations": iters,
                       **_summary(ms, "on", "off"), "classes_off": _classes(paths["off"]), "classes_on": _classes(paths["on"])}
    del bb, paths
    torch.cuda.empty_cache()
    eng = _engine(args.envs)
    ms, iters = _rounds({"off": eng(False), "on": eng(True)}, args.rounds, args.seconds)
    rec["update_step"] = {"config": f"ExtrinsicAdapt.update_step + optimizer step, img + seg + proprioception, {args.envs} envs x "
                                    f"{HORIZON} steps, minibatch {args.envs * HORIZON // MINI_EPOCHS}", "iterations": iters,
                          **_summary(ms, "on", "off")}
    del eng
    torch.cuda.empty_cache()
    if args.parent_root:
        rec["switch_off_against_parent"] = _control(args.parent_root, args.envs, args.rounds, args.seconds)
    else:
        rec["switch_off_against_parent"] = "not measured in this run (no --parent-root)"
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
