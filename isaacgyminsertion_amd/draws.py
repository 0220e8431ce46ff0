"""The seeded draws of the augmentation kernels, restated for the host: csrc/draws.h and csrc/tok_hash.h in torch ops, on
whatever device the element numbers live on.  The one restatement the product uses -- ``TactileAugment`` / ``SyncTransform``
(``draw_seeded``, ``apply*``) and ``PclAugment.apply`` call it; tests/test_draws_cpu.py holds it to the header, to the
compiled tools/draws_check.cpp and to the tests' independent numpy restatement (oracle/token_dropout.py).  Only torch and
numpy: the native library is never loaded from here.

``PLANES`` / ``SITES`` are the table of draws.h, name for name: ONE flat namespace, Gaussian plane p occupying sites 2p and
2p + 1.  To add a site: one line there, one here, one in the test reference that restates the draw."""
import math

import numpy as np
import torch

PLANES = dict(IMG_PLANE_DEPTH=0, IMG_PLANE_MASK=1, TAC_NOISE_PLANE=2,
              PCL_PLANE_PN=3, PCL_PLANE_JITTER=4, PCL_PLANE_FREE=5, PCL_PLANE_CONTOUR=6)
SITES = dict(PCL_SITE_HIT=14, PCL_SITE_ANGLE=15, PCL_SITE_AXIS=16, PCL_SITE_MASK=17, PCL_SITE_CONTOUR=18, PCL_SITE_SIDE=19,
             PCL_SITE_INDEX=20, PCL_SITE_EXEMPT=21, PCL_SITE_DROP=22, TAC_SITE_JITTER=23, TAC_SITE_BRIGHT=24,
             TAC_SITE_CONTRAST=25, TAC_SITE_ROTATE=26, TAC_SITE_ANGLE=27, TAC_SITE_KEEP=28, IMG_SITE_ANGLE=29, IMG_SITE_KEEP=30)

_M32 = 0xFFFFFFFF


def _mul32(x, k):
    """(x * k) mod 2^32 for an int64 tensor of 32-bit values: two 16-bit halves, so no product leaves int64."""
    return ((x & 0xFFFF) * k + ((((x >> 16) * k) & 0xFFFF) << 16)) & _M32


def tok_hash(seed, site, idx):
    """csrc/tok_hash.h on an int64 tensor ``idx`` of element numbers (taken modulo 2^32) -> int64 values below 2^32, on
    idx's device.  ``seed``: a Python int below 2^64, or its two 32-bit words ``(lo, hi)`` where ``hi`` may be an int64
    tensor that broadcasts against ``idx`` (a seed per element: the point cloud's ``seed_episode + (episode << 32)``)."""
    lo, hi = seed if isinstance(seed, tuple) else (int(seed), int(seed) >> 32)
    x = _mul32(idx & _M32, 0x9E3779B1) ^ (lo & _M32) ^ ((site * 0x85EBCA77) & _M32)
    x = _mul32(x ^ (x >> 16), 0x7FEB352D)
    x = _mul32(x ^ (x >> 15), 0x846CA68B)
    x = ((x ^ (x >> 16)) + (hi & _M32)) & _M32
    x = _mul32(x ^ (x >> 15), 0x2C1B3C6D)
    x = _mul32(x ^ (x >> 12), 0x297A2D39)
    return x ^ (x >> 15)


def threshold(p):
    """``draw_threshold``: an event of probability ``p`` is ``hash < threshold(p)`` -- p rounded to float32, times 2^32,
    truncated, as a Python int; p = 1 gives 2^32, above every hash: always."""
    return int(float(np.float32(p)) * 2.0 ** 32) if p > 0 else 0


def u(h):
    """``draw_u``: (h >> 8) 2^-24 in [0, 1), float64 -- exact there and in fp32."""
    return (h >> 8).double() * 2.0 ** -24


def unit(h):
    """``draw_unit``: 2u - 1 in [-1, 1), float64 -- exact there and in fp32."""
    return (h >> 8).double() * 2.0 ** -23 - 1.0


def index(h, n):
    """``draw_index``: floor(u n), int64 in [0, n)."""
    return ((h >> 8) * n) >> 24


def gauss(seed, plane, e, dtype):
    """csrc/aug_gauss.h: the Box-Muller sample of (seed, plane, element) for every element number of ``e``, computed in
    ``dtype`` with the kernel's branch for ln u1 (log below 1/2, log1p of the exact distance from 1 above)."""
    k1, k2 = tok_hash(seed, 2 * plane, e) >> 8, tok_hash(seed, 2 * plane + 1, e) >> 8
    low = torch.log((k1.to(dtype) + 0.5) * 2.0 ** -24)
    high = torch.log1p(-(((0xFFFFFF - k1).to(dtype) + 0.5) * 2.0 ** -24))
    ln_u1 = torch.where(k1 < (1 << 23), low, high)
    return torch.sqrt(-2.0 * ln_u1) * torch.cos((2.0 * math.pi) * (k2.to(dtype) * 2.0 ** -24))


def elements(shape, device=None):
    """The linear index of every element of a tensor of ``shape``, in that shape: the element numbers of its noise."""
    return torch.arange(math.prod(shape), device=device).reshape(shape)


def keep_grid(seed, site, p, shape):
    """The keep cells of ``site`` at elements 0 .. prod(shape) - 1: uint8 of ``shape``, 1 where ``hash >= threshold(p)``."""
    return (tok_hash(seed, site, elements(shape)) >= threshold(p)).to(torch.uint8)
