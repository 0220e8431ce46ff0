"""Float64 restatement of the tactile augmentation (csrc/tactile_augment.h, utils.TactileAugment) -- TEST INFRASTRUCTURE.

Plain torch on the CPU, image by image where the kernel works image by image: the jitter's two clamped lines in float64,
and from tests/img_augment_ref.py the gather and crop by slicing (``window``), the float64 rotation, its tie band, the
Box-Muller over ``oracle.token_dropout.tok_hash`` and the repeated ``keep``.  Every function takes the op's arguments (CPU
tensors; the fp32 parameters are widened exactly) and returns float64.
"""
import numpy as np
import torch

from tests.img_augment_ref import TIE_EPS, TIE_SHARE_MAX, gauss, patch_mask, rotate, tie_band, window  # noqa: F401

NOISE_PLANE = 2          # hash sites 4 and 5; the camera pair holds planes 0 and 1
U = 2.0 ** -24           # fp32 unit roundoff


def jitter_image(x, b, c):
    """One image: x = clamp(x b, 0, 1); m = its mean; x = clamp((x - m) c + m, 0, 1)."""
    x = (x.double() * float(b)).clamp(0, 1)
    m = x.mean()
    return ((x - m) * float(c) + m).clamp(0, 1)


def jitter_images(y, jitter):
    """(n, 1, H, W) float64, (n, 3) = (flag, b, c): a flag of 0 passes the image as it is."""
    out = y.clone()
    for i in range(y.shape[0]):
        if jitter[i, 0] != 0:
            out[i] = jitter_image(y[i], jitter[i, 1], jitter[i, 2])
    return out


def jitter_bound(pixels):
    """Bound on |fp32 kernel - float64 restatement| of one jittered pixel of an image of ``pixels`` pixels, derived from
    the kernel's arithmetic (u = 2^-24, every fp32 operation has a relative error of at most u; b, c in [0.9, 1.1]):
      z = clamp(x b, 0, 1): one product of magnitude <= 1.1 whose clamp (1-Lipschitz, and exact above 1) leaves <= u;
      m = sum(z) / pixels with z >= 0: a term passes through at most ceil(pixels / 256) - 1 sequential additions in its
        thread, 6 butterfly levels in its wave and 3 additions over the four waves -- ``depth`` roundings -- so the sum is
        off by <= depth u sum(z); the inputs' own error adds u and the division one more: dm <= (depth + 2) u, as m <= 1;
      out = clamp((z - m) c + m, 0, 1) = clamp(z c + m (1 - c)): dz enters times c (1.1 u), dm times |1 - c| <= 0.1, the
        subtraction rounds once (|z - m| <= 1: u, times c: 1.1 u), the product once (1.1 u), the sum once (1.1 u).
    Total (4.4 + 0.1 (depth + 2)) u; the factor behind it covers the second-order terms.  2048 pixels: depth 16, 6.2 u =
    3.7e-7.  A sum by one thread (depth 2047) or by atomics in no fixed order has no bound of this size."""
    depth = (-(-pixels // 256) - 1) + 6 + 3
    return (4.4 + 0.1 * (depth + 2)) * U * (1 + 64 * U)


def augment(arena, rows, offsets, jitter, angles, keep, out_h, out_w, patch, noise_std=0.0, seed=0):
    """The op, restated -> (out, band): float64 (B, T, F, 1, out_h, out_w) and the pixels to exclude (rotation ties)."""
    N, T, Fg = arena.shape[:3]
    B = rows.numel()
    y = window(arena, rows, offsets, out_h, out_w)
    y = jitter_images(y, jitter)
    ang = angles.reshape(-1)
    y = torch.where((ang != 0)[:, None, None, None], rotate(y, ang), y)
    if noise_std > 0:
        y = y + float(np.float32(noise_std)) * gauss(seed, NOISE_PLANE, y.shape)
    if keep is not None:
        y = y * patch_mask(keep, out_h, out_w, patch)
    shape = (B, T, Fg, 1, out_h, out_w)
    return y.reshape(shape), tie_band(ang, out_h, out_w).reshape(shape)
