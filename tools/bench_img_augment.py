#!/usr/bin/env python
"""One training batch of the camera pair (depth frames + segmentation masks) through the fused augmentation, beside ATen.

    python tools/bench_img_augment.py [--rounds R] [--iters K] [--root TREE] [--out profiles/img_augment.json]

The batch of the offline student's default configuration: 64 samples, T = 1, arenas of 60 x 104 frames (2048 resident
samples), crop to 54 x 96, rotation 1 degree, Gaussian noise 0.01, patch masking 0.3 (patch 16).
  fused : ``SyncTransform.fused(img_arena, seg_arena, rows)`` -- the CPU draw, three small host-to-device copies and ONE
          launch of k_image_pair_augment;
  aten  : two ``index_select``s, then ``SyncTransform.forward`` -- the same CPU draw and the torch-op composition
          (advanced-index crop, affine_grid + grid_sample, randn noise, repeat_interleave mask) on the device.
Host clock around K iterations ending in a device synchronise, R alternating rounds, medians with min .. max, in ms per
batch.  The record is stamped with the library's build hash.  --root: the tree whose package and library to time
(default: this one), to set another commit's build beside this one in the same job. No bar: the pair is stated in README
as it comes out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "img_augment.json"))
    ap.add_argument("--root", default=ROOT, help="the tree whose package and library to load")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_img_augment: no HIP device (timings are taken on the GPU only)")
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.models.transformer.utils import define_img_transforms
    N, B, T = 2048, 64, 1
    g = torch.Generator().manual_seed(0)
    seg = torch.randint(0, 4, (N, T, 1, 60, 104), generator=g).float().cuda()
    img = torch.rand(N, T, 1, 60, 104, generator=g).cuda() * (seg > 1)
    sync = define_img_transforms(60, 104, 54, 96, 16, 0.01, 0.3, rotation_deg=1.0)[3]
    sync.generator = torch.Generator().manual_seed(1)
    batches = [torch.randperm(N, generator=g)[:B].cuda() for _ in range(16)]

    def fused(i):
        return sync.fused(img, seg, batches[i % 16])

    def aten(i):
        rows = batches[i % 16]
        return sync(img.index_select(0, rows), seg.index_select(0, rows))

    paths = {"fused": fused, "aten": aten}
    for fn in paths.values():                      # warm-up: code loading, clocks
        for i in range(20):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(args.rounds):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.iters):
                fn(i)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.iters)
    med = {k: _median(v) for k, v in ms.items()}
    slower = [r for r in range(args.rounds) if ms["fused"][r] > ms["aten"][r]]
    rec = {
        "tool": "tools/bench_img_augment.py",
        "build": _lib.lib().igi_build_info().decode(),
        "device": torch.cuda.get_device_name(0),
        "config": f"{B} samples x T = {T} from {N} resident 60 x 104 frames, crop 54 x 96, rotation 1 degree, noise 0.01, "
                  f"masking 0.3 (patch 16); host clock around {args.iters} batches ending in a device synchronise (the CPU "
                  f"draw of both paths included); {args.rounds} alternating rounds",
        "ms_per_batch_rounds": {k: [round(t, 4) for t in v] for k, v in ms.items()},
        "ms_per_batch_median": {k: round(v, 4) for k, v in med.items()},
        "ms_per_batch_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "fused_over_aten": round(med["fused"] / med["aten"], 4),
        "rounds_where_fused_is_slower": slower,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
