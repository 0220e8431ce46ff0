"""Float64 restatement of the camera-pair augmentation (csrc/augment.h, utils.SyncTransform) -- TEST INFRASTRUCTURE.

Plain torch on the CPU: slicing for the gather and the crop, ``F.affine_grid`` / ``F.grid_sample`` in float64 for the
rotation, numpy Box-Muller over ``oracle.token_dropout.tok_hash`` for the noise, a repeated ``keep`` for the patch mask.
Every function takes the op's arguments (CPU tensors) and returns float64.

A nearest-neighbour rotation is discontinuous where a source coordinate falls on a rounding tie (k + 1/2): fp32 and
float64 may then pick different neighbours.  ``tie_band`` marks the output pixels whose float64 source coordinate lies
within ``TIE_EPS`` of a tie on either axis; comparisons exclude exactly those, and the tests bound their share.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.token_dropout import tok_hash

TIE_EPS = 1e-4
TIE_SHARE_MAX = 0.005
# the rotation cases of tests/test_gpu_img_augment.py: (out_h, out_w) and one angle per sample, (image, mask) in degrees
ROT_SIZES = [(54, 96), (17, 23)]
ROT_ANGLES_DEG = [(0.0, 0.0), (1.0, 1.0), (0.0, -1.0), (-0.37, 3.0), (3.0, -0.37)]


def rot_angles():
    """fp32 (5, 2) radians, as the op receives them."""
    return (torch.tensor(ROT_ANGLES_DEG, dtype=torch.float64) * (math.pi / 180)).float()


def window(x, rows, offsets, out_h, out_w):
    """Gather + crop: (N, ..., Hs, Ws), `planes` images per sample -> (B*planes, 1, out_h, out_w) float64, every image
    with its own (top, left) row of ``offsets`` (B*planes, 2).  A sample number outside [0, N) and every position outside
    the stored frame read as 0."""
    N, (Hs, Ws) = x.shape[0], x.shape[-2:]
    frames = x.reshape(N, -1, Hs, Ws)
    planes = frames.shape[1]
    out = torch.zeros(rows.numel() * planes, 1, out_h, out_w, dtype=torch.float64)
    for i in range(out.shape[0]):
        b, plane = divmod(i, planes)
        r, top, left = int(rows[b]), int(offsets[i, 0]), int(offsets[i, 1])
        if not 0 <= r < N:
            continue
        y0, y1 = max(top, 0), min(top + out_h, Hs)
        x0, x1 = max(left, 0), min(left + out_w, Ws)
        if y0 < y1 and x0 < x1:
            out[i, 0, y0 - top:y1 - top, x0 - left:x1 - left] = frames[r, plane, y0:y1, x0:x1].double()
    return out


def sample_window(x, rows, offsets, out_h, out_w):
    """The camera's case of ``window``: (N, T, 1, Hs, Ws) and one (top, left) per SAMPLE -> (B, T, 1, out_h, out_w)."""
    T = x.shape[1]
    return window(x, rows, offsets.repeat_interleave(T, 0), out_h, out_w).reshape(rows.numel(), T, 1, out_h, out_w)


def _theta(ang, H, W):
    ang = ang.double()
    cos, sin = torch.cos(ang), torch.sin(ang)
    zero = torch.zeros_like(cos)
    return torch.stack([torch.stack([cos, -sin * H / W, zero], 1), torch.stack([sin * W / H, cos, zero], 1)], 1)


def source_coords(ang, H, W):
    """(n,) radians -> float64 (n, H, W, 2): the (x, y) source pixel coordinate grid_sample(align_corners=False) reads."""
    grid = F.affine_grid(_theta(ang, H, W), [ang.numel(), 1, H, W], align_corners=False)
    return torch.stack([((grid[..., 0] + 1) * W - 1) / 2, ((grid[..., 1] + 1) * H - 1) / 2], -1)


def tie_band(ang, H, W, eps=TIE_EPS):
    """bool (n, H, W): the source coordinate is within ``eps`` of k + 1/2 on either axis.  Angle 0 has no band (the kernel
    copies; the coordinates are integers)."""
    c = source_coords(ang, H, W)
    frac = c - torch.floor(c)
    near = ((frac - 0.5).abs() <= eps).any(-1)
    return near & (ang != 0)[:, None, None]


def rotate(x, ang):
    """(n, 1, H, W) float64, (n,) radians -> rotated about the centre: nearest, zero fill."""
    H, W = x.shape[-2:]
    grid = F.affine_grid(_theta(ang, H, W), list(x.shape), align_corners=False)
    return F.grid_sample(x.double(), grid, mode='nearest', padding_mode='zeros', align_corners=False)


def gauss(seed, plane, shape):
    """z of every element of an output tensor of ``shape``: float64 Box-Muller over the two hashes of (seed, plane, e)."""
    e = np.arange(int(np.prod(shape)), dtype=np.uint64)
    h1, h2 = tok_hash(seed, 2 * plane, e), tok_hash(seed, 2 * plane + 1, e)
    u1 = ((h1 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = (h2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
    return torch.from_numpy(z).reshape(shape)


def threshold(p):
    """csrc/draws.h ``draw_threshold``: p rounded to fp32, times 2^32, truncated, kept in 64 bits (p = 1: always)."""
    return int(float(np.float32(p)) * 2.0 ** 32) if p > 0 else 0


def _hash(seed, site, n):
    """The hashes of elements 0 .. n - 1 of ``site``, int64."""
    return tok_hash(int(seed), site, np.arange(n, dtype=np.uint64)).astype(np.int64)


def _unit(seed, site, n):
    """2u - 1, u = (h >> 8) 2^-24, of the same elements: float64, exact."""
    return (_hash(seed, site, n) >> 8).astype(np.float64) * 2.0 ** -23 - 1.0


def patch_mask(keep, out_h, out_w, patch):
    """uint8 (n, gh, gw) -> float64 (n, 1, out_h, out_w): the multiplier of every pixel (1 past the last whole patch)."""
    n, gh, gw = keep.shape
    m = torch.ones(n, 1, out_h, out_w, dtype=torch.float64)
    m[:, 0, :gh * patch, :gw * patch] = keep.double().repeat_interleave(patch, 1).repeat_interleave(patch, 2)
    return m


def augment(img, seg, rows, offsets, angles, keep, out_h, out_w, patch, noise_std=0.0, seed=0):
    """The op, restated: -> (img_out, seg_out, band) with band bool (2, B, T, 1, out_h, out_w): pixels to exclude."""
    B, T = rows.numel(), img.shape[1]
    outs, bands = [], []
    for k, x in enumerate((img, seg)):
        ang = angles[:, k].repeat_interleave(T)
        y = window(x, rows, offsets.repeat_interleave(T, 0), out_h, out_w)
        y = torch.where((ang != 0)[:, None, None, None], rotate(y, ang), y)
        if noise_std > 0:
            y = y + float(np.float32(noise_std)) * gauss(seed, k, y.shape)
        if k == 0 and keep is not None:
            y = y * patch_mask(keep, out_h, out_w, patch)
        outs.append(y.reshape(B, T, 1, out_h, out_w))
        bands.append(tie_band(ang, out_h, out_w).reshape(B, T, 1, out_h, out_w))
    return outs[0], outs[1], torch.stack(bands)
