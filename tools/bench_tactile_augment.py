#!/usr/bin/env python
"""One training batch of tactile images through the fused augmentation, beside today's torch path.

    python tools/bench_tactile_augment.py [--rounds R] [--iters K] [--root TREE] [--out profiles/tactile_augment.json]

The batch of the offline student: 64 samples, T = 1, 3 fingers, 32 x 64 frames in [-1, 1] (2048 resident samples), in two
configurations:
  stock         : Gaussian noise 0.001, no crop, no masking (the default config with ``use_tactile``);
  everything on : crop 4 / 8 (to 28 x 56), noise 0.001, masking 0.3 with patch 8.
  fused : ``TactileAugment.fused(arena, rows, generator)`` -- the CPU draw, ONE host-to-device copy of the packed
          parameters and ONE launch of k_tactile_augment;
  torch : ``index_select``, then the ``nn.Sequential`` of ``define_tactile_transforms`` (``_Crop`` + ``_TrainAugment`` +
          ``GaussianNoise`` + ``Masking``) on the device, as ``ResidentLoader`` calls it -- code from before the fused path.
Host clock around K iterations ending in a device synchronise, R alternating rounds, medians with min .. max, in ms per
batch.  The record is stamped with the library's build hash.  --root: the tree whose package and library to time
(default: this one), to set another commit's build beside this one in the same job. No bar: the pairs are stated in
README as they come out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {"stock": dict(crop=(32, 64), noise=0.001, masking=0.0, patch=16),
           "everything_on": dict(crop=(28, 56), noise=0.001, masking=0.3, patch=8)}


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tactile_augment.json"))
    ap.add_argument("--root", default=ROOT, help="the tree whose package and library to load")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tactile_augment: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.models.transformer.utils import define_tactile_augment, define_tactile_transforms
    N, B, T, Fg = 2048, 64, 1, 3
    g = torch.Generator().manual_seed(0)
    arena = (torch.rand(N, T, Fg, 1, 32, 64, generator=g) * 2 - 1).cuda()
    batches = [torch.randperm(N, generator=g)[:B].cuda() for _ in range(16)]
    results = {}
    for name, c in CONFIGS.items():
        aug = define_tactile_augment(32, 64, *c["crop"], c["patch"], c["noise"], c["masking"])[0]
        seq = define_tactile_transforms(32, 64, *c["crop"], c["patch"], c["noise"], c["masking"])[0].cuda()
        gen = torch.Generator().manual_seed(1)

        def fused(i):
            return aug.fused(arena, batches[i % 16], gen)

        def torch_path(i):
            x = arena.index_select(0, batches[i % 16])
            y = seq(x.reshape(-1, 1, 32, 64))
            return y.reshape(B, T, Fg, 1, *y.shape[2:])

        paths = {"fused": fused, "torch": torch_path}
        for fn in paths.values():                      # warm-up: code loading, kernel selection, clocks
            for i in range(20):
                fn(i)
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    fn(i)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.iters)
        med = {k: _median(v) for k, v in ms.items()}
        results[name] = {
            "config": f"crop to {c['crop'][0]} x {c['crop'][1]}, noise {c['noise']}, masking {c['masking']} (patch {c['patch']})",
            "ms_per_batch_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "ms_per_batch_median": {k: round(v, 4) for k, v in med.items()},
            "ms_per_batch_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "fused_over_torch": round(med["fused"] / med["torch"], 4),
            "rounds_where_fused_is_slower": [r for r in range(args.rounds) if ms["fused"][r] > ms["torch"][r]],
        }
    rec = {
        "tool": "tools/bench_tactile_augment.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "batch": f"{B} samples x T = {T} x {Fg} fingers from {N} resident 32 x 64 frames; host clock around {args.iters} "
                 f"batches ending in a device synchronise (the CPU draw and the host-to-device copy of the fused path "
                 f"included); {args.rounds} alternating rounds",
        "configurations": results,
    }
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
