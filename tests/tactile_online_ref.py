"""Float64 restatement of the SEEDED draws of the online student's tactile augmentation (csrc/tactile_augment_seeded.h,
utils.TactileAugment.draw_seeded / fused_seeded) -- TEST INFRASTRUCTURE, layered on tests/tactile_augment_ref.py.

The draws are numpy over ``oracle.token_dropout.tok_hash`` (an implementation of the hash apart from the package's torch
one): flags and keep cells are integer comparisons; the two factors and the angle are float64 arithmetic on exact operands
(2u - 1 = k 2^-23 - 1 is exact; its product with an fp32 constant has 48 bits; adding 1 leaves 51) rounded ONCE to fp32,
which is what the kernel's single fp32 fmaf / multiply gives.  The image chain is ``tactile_augment_ref.augment`` with the
window at (0, 0).

``CASES`` are the shapes of tests/test_gpu_tactile_online.py; ``SEEDS`` were chosen on the CPU so that, for every case, at
most ``TIE_SHARE_MAX`` of the output pixels have a rotated source coordinate within 1e-4 of a rounding tie
(tests/test_tactile_online_cpu.py asserts it from this file alone).
"""
import math

import numpy as np
import torch

from tests import tactile_augment_ref as R
from tests.img_augment_ref import _hash, _unit, threshold  # noqa: F401  (the tests reach them through this module)

SITES = dict(JITTER=23, BRIGHT=24, CONTRAST=25, ROTATE=26, ANGLE=27, KEEP=28)
JITTER_P, ROTATE_P, JITTER, ROTATE_DEG = 0.3, 0.5, 0.1, 3.0
TIE_SHARE_MAX = 0.001
ARENA_ROWS = 6                                           # T * N of the GPU tests' arenas
ROWS = [4, 0, 5, 4, ARENA_ROWS]                          # one repeated row, one outside the arena
# (history, fingers, H, W, patch): 8 pixels per thread and 16-byte stores; fewer pixels than threads, scalar stores and a
# partial last patch; the square frame
CASES = [(1, 3, 32, 64, 16), (2, 3, 32, 64, 8), (1, 3, 9, 13, 4), (2, 3, 9, 13, 4), (1, 3, 64, 64, 16)]
MANY = (67, 1, 1, 32, 64, 16)                            # one case of 67 images: B = 67 rows of one plane
SEEDS = [3, 0x1234567890ABCDEF & (2 ** 63 - 1), 2 ** 63 - 2]
EDGE_SEED = 11                                           # the one image of 64 x 128 = 8192 pixels: jittered and turned
# the trainer cases: 8 envs x 4 steps in 4 minibatches of 8 rows x 3 fingers, 4 mini-epochs = 16 optimizer steps per epoch;
# the step seeds are the stream of a private generator seeded cfg.seed (42)
ENGINE = dict(envs=8, horizon=4, mini_epochs=4, seed=42)


def draws(n_images, seed, out_h, out_w, patch, masking_prob):
    """-> (offsets int32 (n, 2) zeros, jitter fp32 (n, 3), angles fp32 (n,), keep uint8 (n, gh, gw) or None)."""
    n = int(n_images)
    on = _hash(seed, SITES["JITTER"], n) < threshold(JITTER_P)
    turn = _hash(seed, SITES["ROTATE"], n) < threshold(ROTATE_P)
    amp, rad = float(np.float32(JITTER)), float(np.float32(ROTATE_DEG * math.pi / 180))
    b = np.where(on, (_unit(seed, SITES["BRIGHT"], n) * amp + 1.0).astype(np.float32), np.float32(1))
    c = np.where(on, (_unit(seed, SITES["CONTRAST"], n) * amp + 1.0).astype(np.float32), np.float32(1))
    ang = np.where(turn, (_unit(seed, SITES["ANGLE"], n) * rad).astype(np.float32), np.float32(0))
    jitter = torch.from_numpy(np.stack([on.astype(np.float32), b.astype(np.float32), c.astype(np.float32)], 1))
    gh, gw = out_h // patch, out_w // patch
    keep = None
    if masking_prob > 0 and gh * gw > 0:
        kept = _hash(seed, SITES["KEEP"], n * gh * gw) >= threshold(masking_prob)
        keep = torch.from_numpy(kept.astype(np.uint8)).reshape(n, gh, gw)
    return torch.zeros(n, 2, dtype=torch.int32), jitter, torch.from_numpy(ang.astype(np.float32)), keep


def packed(offsets, jitter, angles):
    """The draws as the op's ``draws`` output: int32 (n, 6) = 0, 0, flag, bits of (b, c, angle)."""
    bits = lambda t: torch.from_numpy(t.numpy().astype(np.float32).view(np.int32).copy())   # noqa: E731
    return torch.stack([offsets[:, 0], offsets[:, 1], (jitter[:, 0] != 0).to(torch.int32), bits(jitter[:, 1]),
                        bits(jitter[:, 2]), bits(angles)], 1)


def augment(arena, rows, seed, patch, noise_std=0.0, masking_prob=0.0):
    """The op, restated: ``arena`` (R, T, F, 1, H, W) on the CPU -> (out float64 (B, T, F, 1, H, W), band, the draws)."""
    H, W = arena.shape[-2:]
    n = rows.numel() * arena.shape[1] * arena.shape[2]
    off, jit, ang, keep = draws(n, seed, H, W, patch, masking_prob)
    out, band = R.augment(arena, rows, off, jit, ang, keep, H, W, patch, noise_std, seed)
    return out, band, (off, jit, ang, keep)


def tie_share(n_images, seed, H, W):
    """The share of the n_images * H * W output pixels whose rotated source coordinate is within 1e-4 of a tie."""
    _off, _jit, ang, _keep = draws(n_images, seed, H, W, 1, 0.0)
    return float(R.tie_band(ang, H, W).double().mean())


def engine_seeds(k, seed=ENGINE["seed"]):
    """The first ``k`` step seeds of a trainer built from a config with ``seed``."""
    g = torch.Generator().manual_seed(seed)
    return [int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g)) for _ in range(k)]


def arena(T, Fg, H, W, seed=0, rows=ARENA_ROWS):
    return torch.rand(rows, T, Fg, 1, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1
