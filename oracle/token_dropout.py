"""The token encoder's dropout masks, recomputed on the host -- TEST INFRASTRUCTURE, never imported by the product.

csrc/token_encoder.h drops with a counter-based hash: an element is KEPT iff ``tok_hash(seed, site, element) >= thresh``
with ``thresh = (unsigned)(double(p) * 2^32)`` (``p`` a float32, ``make_drop``), and a kept value is scaled by 1/(1-p).
``seed`` is the one ``torch.randint(0, 2**62, (1,))`` draw ``HipTransformerEncoder.forward`` takes from torch's CPU
generator, so every mask of a training step can be restated exactly here, in numpy ``uint32`` arithmetic, and handed to
``oracle.student.encoder_layer(..., masks=...)`` as constants: the float64 autograd of that restatement is then the
reference for the train-mode output and every train-mode gradient of the HIP kernels.

Sites and element numbers (those of the header, layer ``l`` of the stack, d_model = 32, H heads, ff hidden units):

  site 4 l + 0  attention probabilities   element ((b * H + h) * S + i) * S + j     mask (B, H, S, S)
  site 4 l + 1  self-attention branch     element row * 32 + f,  row = b * S + s     mask (B, S, 32)
  site 4 l + 2  GELU output               element row * ff + c                       mask (B, S, ff)
  site 4 l + 3  feed-forward branch       element row * 32 + f                       mask (B, S, 32)

Element numbers are taken modulo 2^32, as the kernels' ``(unsigned int)`` casts of their 64-bit indices do; no test size
comes near 2^32 elements, so the wrap is stated, not exercised.
"""
import numpy as np

D_MODEL = 32
SITE_ATTN, SITE_SA, SITE_FF_ACT, SITE_FF = 0, 1, 2, 3


def tok_hash(seed, site, idx):
    """token_encoder.h ``tok_hash``: ``seed`` a Python int below 2^64, ``site`` an int, ``idx`` an integer array (taken
    modulo 2^32).  Returns uint32 of idx's shape."""
    seed = int(seed)
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    idx = (np.asarray(idx).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = idx * np.uint32(0x9E3779B1) ^ lo ^ np.uint32((int(site) * 0x85EBCA77) & 0xFFFFFFFF)
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
        x = x + hi
        x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x2C1B3C6D)
        x = x ^ (x >> np.uint32(12)); x = x * np.uint32(0x297A2D39)
        x = x ^ (x >> np.uint32(15))
    return x


def threshold(p):
    """``make_drop``: p is rounded to float32 BEFORE the double(p) * 2^32 truncation (0.1 -> 429496736)."""
    return np.uint32(int(float(np.float32(p)) * 2.0 ** 32)) if p > 0 else np.uint32(0)


def keep_scale(p, seed, site, idx):
    """float64 array of idx's shape: 0 where the element is dropped, 1/(1-p) where it is kept (p as the float32 the kernels
    receive); all ones for p == 0."""
    idx = np.asarray(idx)
    if not p > 0:
        return np.ones(idx.shape, dtype=np.float64)
    keep = tok_hash(seed, site, idx) >= threshold(p)
    return keep.astype(np.float64) / (1.0 - float(np.float32(p)))


def layer_masks(B, S, H, ff, p, seed, l):
    """The four masks of layer ``l`` as float64 numpy arrays, in the shapes ``oracle.student.encoder_layer`` multiplies
    with: (attention (B, H, S, S), self-attention branch (B, S, 32), GELU output (B, S, ff), feed-forward branch
    (B, S, 32))."""
    att = np.arange(B * H * S * S, dtype=np.uint64).reshape(B, H, S, S)       # ((b * H + h) * S + i) * S + j
    row = np.arange(B * S * D_MODEL, dtype=np.uint64).reshape(B, S, D_MODEL)  # row * 32 + f
    hid = np.arange(B * S * ff, dtype=np.uint64).reshape(B, S, ff)            # row * ff + c
    return (keep_scale(p, seed, 4 * l + SITE_ATTN, att), keep_scale(p, seed, 4 * l + SITE_SA, row),
            keep_scale(p, seed, 4 * l + SITE_FF_ACT, hid), keep_scale(p, seed, 4 * l + SITE_FF, row))


def stack_masks(B, S, H, ff, p, seed, layers, dtype=None):
    """``layer_masks`` of every layer of a stack as torch tensors (float64 unless ``dtype``): what ``oracle.student.decode``
    takes as ``masks``."""
    import torch
    return [tuple(torch.from_numpy(m).to(dtype or torch.float64) for m in layer_masks(B, S, H, ff, p, seed, l))
            for l in range(layers)]
