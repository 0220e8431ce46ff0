"""Float64 restatement of the SEEDED draws of the online student's camera-pair augmentation (csrc/augment_seeded.h,
utils.SyncTransform.draw_seeded / fused_seeded) -- TEST INFRASTRUCTURE, layered on tests/img_augment_ref.py.

The draws are numpy over ``oracle.token_dropout.tok_hash`` (an implementation of the hash apart from the package's torch
one): keep cells are integer comparisons; an angle is float64 arithmetic on exact operands (2u - 1 = k 2^-23 - 1 is exact;
its product with the fp32 ``max_rad`` has 48 bits) rounded ONCE to fp32, which is what the kernel's single fp32 multiply
gives.  The pixel chain is ``img_augment_ref.augment`` with the window at (0, 0) and the output at the stored size.

``CASES`` are the shapes of tests/test_gpu_img_online.py; ``SEEDS`` -- one table, imported by both test files -- were chosen
on the CPU so that, for every (seed, size, rotation_deg) of the GPU tests, at most ``TIE_SHARE_MAX`` of the output pixels
have a rotated source coordinate within 1e-4 of a rounding tie (tests/test_img_online_cpu.py asserts it from this file
alone).  The rotations are sized to the frames: a turn moves a pixel only where (extent / 2) sin(angle) passes 1/2, so the
smaller frames get the larger ``rotation_deg``.
"""
import math

import numpy as np
import torch

from tests import img_augment_ref as A
from tests.img_augment_ref import _hash, _unit, threshold  # noqa: F401  (the tests reach them through this module)

SITES = {"ANGLE": 29, "KEEP": 30}
TIE_SHARE_MAX = 0.001
ARENA_ROWS = 6                                           # horizon * envs of the GPU tests' arenas
ROWS = [4, 0, 5, 4, ARENA_ROWS]                          # one repeated row, one outside the arena
# (T, H, W, patch, rotation_deg): two bands and 16-byte stores; the odd width -- scalar stores, a partial last group, partial
# patches at patch 4, a 1 x 1 grid at patch 16; a cell per pixel
CASES = [(1, 54, 96, 16, 1.0), (2, 54, 96, 16, 1.0), (1, 17, 23, 4, 10.0), (2, 17, 23, 16, 10.0), (2, 8, 8, 1, 20.0)]
MANY = (67, 1, 17, 23, 4, 10.0)                          # B = 67 at 17 x 23
SEEDS = [5, 0x0FEDCBA987654321, 2 ** 63 - 2]
# the trainer cases: 8 envs x 4 steps in 4 minibatches of 8 rows, 4 mini-epochs = 16 optimizer steps per epoch; frames of
# 54 x 96, T = 1; the step seeds are the stream of a private generator seeded cfg.seed (42)
ENGINE = dict(envs=8, horizon=4, mini_epochs=4, seed=42, hw=(54, 96), rotation_deg=1.0, noise_std=0.01, masking_prob=0.3,
              patch=16)


def max_rad(rotation_deg):
    """The fp32 the kernel is handed, as a Python float: the product in double, rounded once."""
    return float(np.float32(rotation_deg * math.pi / 180))


def draws(B, T, seed, H, W, patch, masking_prob, rotation_deg):
    """-> (offsets int32 (B, 2) zeros, angles fp32 (B, 2): depth, mask; keep uint8 (B*T, gh, gw) or None)."""
    B, T = int(B), int(T)
    ang = np.zeros(2 * B, dtype=np.float32)
    if rotation_deg > 0:
        ang = (_unit(seed, SITES["ANGLE"], 2 * B) * max_rad(rotation_deg)).astype(np.float32)
    gh, gw = H // patch, W // patch
    keep = None
    if masking_prob > 0 and gh * gw > 0:
        kept = _hash(seed, SITES["KEEP"], B * T * gh * gw) >= threshold(masking_prob)
        keep = torch.from_numpy(kept.astype(np.uint8)).reshape(B * T, gh, gw)
    return torch.zeros(B, 2, dtype=torch.int32), torch.from_numpy(ang.reshape(B, 2).copy()), keep


def angle_bits(angles):
    """The draws as the op's ``draws`` output: int32 (B, 2), the bit patterns of the two angles."""
    return torch.from_numpy(angles.numpy().astype(np.float32).view(np.int32).copy())


def augment(img, seg, rows, seed, patch, noise_std=0.0, masking_prob=0.0, rotation_deg=0.0):
    """The op, restated: ``img`` / ``seg`` (R, T, 1, H, W) on the CPU, either may be None -> (img_out, seg_out, band, the
    draws): float64 (B, T, 1, H, W) or None, band bool (2, B, T, 1, H, W).  The draws of a tensor, its noise included, do not
    depend on whether the other is there."""
    some = img if img is not None else seg
    T, (H, W) = some.shape[1], some.shape[-2:]
    off, ang, keep = draws(rows.numel(), T, seed, H, W, patch, masking_prob, rotation_deg)
    blank = torch.zeros_like(some)
    oi, os_, band = A.augment(img if img is not None else blank, seg if seg is not None else blank, rows, off, ang, keep, H, W,
                              patch, noise_std, int(seed))
    return (oi if img is not None else None), (os_ if seg is not None else None), band, (off, ang, keep)


def tie_share(B, seed, H, W, rotation_deg):
    """The share of the B * 2 * H * W output pixels of one frame per (sample, tensor) -- its T frames share the angle --
    whose rotated source coordinate is within 1e-4 of a tie."""
    _off, ang, _keep = draws(B, 1, seed, H, W, 1, 0.0, rotation_deg)
    return float(A.tie_band(ang.reshape(-1), H, W).double().mean())


def engine_seeds(k, seed=ENGINE["seed"]):
    """The first ``k`` step seeds of a trainer built from a config with ``seed``."""
    g = torch.Generator().manual_seed(seed)
    return [int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g)) for _ in range(k)]


def arena(T, H, W, seed=0, rows=ARENA_ROWS):
    return torch.rand(rows, T, 1, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1
