#!/usr/bin/env python
"""Bit dump of the two augmentation ops and of the draws behind them, to compare two builds in separate, fresh processes:

    python tools/augment_dump.py OUT.json [--root TREE] [--draws]

Builds fixed seeded inputs on the CPU, calls torch.ops.mi355ppo.image_pair_augment and tactile_augment over CASES (the
smallest shapes that reach every branch of k_image_pair_augment and k_tactile_augment: 16-byte and scalar stores, a partial
last group of four, two bands per plane, a remainder band of the patch grid, samples and windows outside the arena, the
staged and the direct tactile path) and writes the SHA-256 digest of every output tensor per case.  Neither kernel has
atomics and the tactile mean is summed in a fixed order, so two builds that compute the same thing give the same digests:
tests/test_gpu_augment_bits.py holds this tree to tests/golden/augment_bits.json.
--draws: no GPU; the digests of what ``SyncTransform.draw``, ``SyncEvalTransform.draw`` and ``TactileAugment.draw`` return
from seeded generators, stages on and each stage off in turn, and the number the generator gives next (an extra or a missing
draw moves it): tests/test_augment_draws_cpu.py holds this tree to tests/golden/augment_draws.json.
--root: the tree whose package and library to load (default: this one)."""
import argparse
import hashlib
import json
import math
import os
import sys

SEED = 0x1234567890ABCDEF & (2 ** 63 - 1)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
# camera: (image, mask) degrees per sample -- an angle of 0 and a sample that turns its mask only (tests/img_augment_ref.py)
CAM_ANGLES_DEG = [(0.0, 0.0), (1.0, 1.0), (0.0, -1.0), (-0.37, 3.0), (3.0, -0.37)]
CAM_ROWS = [3, 0, 6, 3, 5]
CAM_OFFSETS = {(60, 104): [[0, 0], [6, 8], [3, 4], [1, 7], [5, 2]], (19, 27): [[0, 0], [2, 4], [1, 3], [2, 0], [0, 4]]}
CAM_OUTSIDE = dict(rows=[2, 7, 4, -1, 2], offsets=[[-3, -5], [10, 20], [2, 4], [-40, 0], [INT_MAX, INT_MIN]])
# name: stored size, output size, T, patch, every stage on?, rows / offsets outside the arena?
CAMERA = {"cam_54x96_on": ((60, 104), (54, 96), 2, 16, True, False),       # 16-byte stores, two bands, 54 = 3 * 16 + 6
          "cam_17x23_on": ((19, 27), (17, 23), 1, 4, True, False),         # scalar stores, a partial last group
          "cam_17x23_outside": ((19, 27), (17, 23), 1, 4, True, True),
          "cam_54x96_off": ((60, 104), (54, 96), 2, 16, False, False)}
TAC_ARENA, TAC_ROWS = (7, 2, 3, 1, 32, 64), [3, 0, 6, 3, 7]
TAC_ANGLES_DEG = [0, 3, -3, 1.7, -0.37, 2.5, -1, 0.05]
TAC_OUTSIDE = dict(rows=[3, -1, 6, 3, 2], offsets={2: [-3, -5], 3: [28, 60], 5: [INT_MAX, INT_MIN]})
# name: output size, patch, every stage on?, rows / offsets outside the arena?
TACTILE = {"tac_32x64_on": ((32, 64), 16, True, False), "tac_28x56_on": ((28, 56), 8, True, False),
           "tac_9x13_on": ((9, 13), 4, True, False), "tac_9x13_off": ((9, 13), 4, False, False),
           "tac_9x13_outside": ((9, 13), 4, True, True)}
CASES = list(CAMERA) + list(TACTILE)
DRAW_SEEDS = (0, 1, 12345)


def _sha(t):
    if t is None:
        return "none"
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode() + t.numpy().tobytes()).hexdigest()


def _keep(n, out, patch, g):
    import torch
    keep = (torch.rand(n, out[0] // patch, out[1] // patch, generator=g) >= 0.3).to(torch.uint8)
    assert 0 < keep.sum() < keep.numel()
    return keep


def camera_inputs(name):
    """The op's arguments of a camera case, on the CPU."""
    import torch
    stored, out, T, patch, on, outside = CAMERA[name]
    g = torch.Generator().manual_seed(sorted(CAMERA).index(name))
    seg = torch.randint(0, 4, (7, T, 1, *stored), generator=g).float()
    img = torch.rand(7, T, 1, *stored, generator=g) + 0.25
    rows = torch.tensor(CAM_OUTSIDE["rows"] if outside else CAM_ROWS)
    offsets = torch.tensor(CAM_OUTSIDE["offsets"] if outside else CAM_OFFSETS[stored], dtype=torch.int32)
    angles = (torch.tensor(CAM_ANGLES_DEG, dtype=torch.float64) * (math.pi / 180)).float()
    if not on:
        return img, seg, rows, offsets, torch.zeros(5, 2), None, *out, 1, 0.0, 0
    return img, seg, rows, offsets, angles, _keep(5 * T, out, patch, g), *out, patch, 0.01, SEED


def tactile_inputs(name):
    """(arena, rows, offsets, jitter, angles, keep, out_h, out_w, patch, noise_std, seed) of a tactile case, on the CPU; a
    case with its stages on holds images of all four kinds (jittered or not) x (rotated or not): the path through LDS and
    the direct one."""
    import torch
    out, patch, on, outside = TACTILE[name]
    n = len(TAC_ROWS) * TAC_ARENA[1] * TAC_ARENA[2]
    g = torch.Generator().manual_seed(100 + sorted(TACTILE).index(name))
    arena = torch.rand(*TAC_ARENA, generator=g) * 2 - 1
    rows = torch.tensor(TAC_OUTSIDE["rows"] if outside else TAC_ROWS)
    offsets = torch.stack([torch.randint(0, 32 - out[0] + 1, (n,), generator=g),
                           torch.randint(0, 64 - out[1] + 1, (n,), generator=g)], 1).to(torch.int32)
    if outside:
        for i, o in TAC_OUTSIDE["offsets"].items():
            offsets[i] = torch.tensor(o, dtype=torch.int32)
    jitter = torch.ones(n, 3)
    jitter[:, 0] = 0
    if not on:
        return arena, rows, offsets, jitter, torch.zeros(n), None, *out, 1, 0.0, 0
    jitter[0::3, 0] = 1
    jitter[0::3, 1:] = 0.9 + 0.2 * torch.rand(len(jitter[0::3]), 2, generator=g)
    deg = torch.tensor([TAC_ANGLES_DEG[i % 8] for i in range(n)], dtype=torch.float64)
    angles = (deg * (math.pi / 180)).float()
    kinds = {(bool(j), bool(a)) for j, a in zip(jitter[:, 0] != 0, angles != 0)}
    assert len(kinds) == 4, kinds
    return arena, rows, offsets, jitter, angles, _keep(n, out, patch, g), *out, patch, 0.05, SEED


def run_case(name):
    """{output name: digest} of one case, through torch.ops.mi355ppo."""
    import torch
    import isaacgyminsertion_amd.ops  # noqa: F401  (registers torch.ops.mi355ppo)
    dev = lambda t: t.cuda() if isinstance(t, torch.Tensor) else t
    if name in CAMERA:
        img, seg = torch.ops.mi355ppo.image_pair_augment(*map(dev, camera_inputs(name)))
        torch.cuda.synchronize()
        return {"img": _sha(img), "seg": _sha(seg)}
    from isaacgyminsertion_amd.algo.models.transformer.utils import TactileAugment
    arena, rows, offsets, jitter, angles, *rest = tactile_inputs(name)
    out = torch.ops.mi355ppo.tactile_augment(*map(dev, (arena, rows, TactileAugment.pack(offsets, jitter, angles), *rest)))
    torch.cuda.synchronize()
    return {"out": _sha(out)}


def draw_configs():
    """{name: zero-argument function -> (the transform, draw's positional arguments)}: stages on, each stage off in turn."""
    from isaacgyminsertion_amd.algo.models.transformer import utils as U
    cam = dict(on=(60, 104, 54, 96, 16, 0.01, 0.3, 1.0), no_crop=(54, 96, 54, 96, 16, 0.01, 0.3, 1.0),
               no_noise=(60, 104, 54, 96, 16, 0.0, 0.3, 1.0), no_masking=(60, 104, 54, 96, 16, 0.01, 0.0, 1.0),
               no_rotation=(60, 104, 54, 96, 16, 0.01, 0.3, 0.0))
    tac = dict(on=(32, 64, 28, 56, 8, 0.001, 0.3), no_crop=(32, 64, 32, 64, 8, 0.001, 0.3),
               no_noise=(32, 64, 28, 56, 8, 0.0, 0.3), no_masking=(32, 64, 28, 56, 8, 0.001, 0.0))
    out = {}
    for k, a in cam.items():
        out[f"sync_{k}"] = lambda a=a: (U.define_img_transforms(*a[:7], rotation_deg=a[7])[3], (3, 2))
    out["sync_eval"] = lambda: (U.define_img_transforms(*cam["on"][:7], rotation_deg=1.0)[4], (3, 2))
    for k, a in tac.items():
        out[f"tactile_{k}"] = lambda a=a: (U.define_tactile_augment(*a)[0], (18,))
    out["tactile_eval"] = lambda: (U.define_tactile_augment(*tac["on"])[1], (18,))
    return out


def run_draw(make):
    """{seed: {"draws": [digest of every tensor / the seed itself], "next": the generator's next number}}"""
    import torch
    out = {}
    for k in DRAW_SEEDS:
        tf, args = make()
        g = torch.Generator().manual_seed(k)
        drawn = tf.draw(*args, g)
        out[str(k)] = {"draws": [d if isinstance(d, int) else _sha(d) for d in drawn],
                       "next": torch.rand(1, generator=g, dtype=torch.float64).item().hex()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--draws", action="store_true", help="the draws' digests (CPU) instead of the ops' (GPU)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))    # the package and its library are --root's
    import isaacgyminsertion_amd
    assert os.path.abspath(isaacgyminsertion_amd.__file__).startswith(os.path.abspath(args.root) + os.sep)
    if args.draws:
        rec = {"tool": "tools/augment_dump.py --draws", "cases": {k: run_draw(f) for k, f in draw_configs().items()}}
    else:
        from isaacgyminsertion_amd import _lib
        rec = {"tool": "tools/augment_dump.py", "cases": {name: run_case(name) for name in CASES}}
        rec["build"] = _lib.lib().igi_build_info().decode()    # after the first op call: torch's HIP runtime loads first
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(rec['cases'])} cases{'' if args.draws else ': ' + rec['build']} -> {args.out}")


if __name__ == "__main__":
    main()
