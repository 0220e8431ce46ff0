"""Tactile image transforms with the reference's names (algo/models/transformer/utils.py:131-278,
457-466): ``define_tactile_transforms`` -> (train transform, eval transform), ``TactileTransform``,
``GaussianNoise``, ``Masking``, ``set_seed``.

The reference builds these from torchvision (absent here) and applies them one image at a time in a Python
loop (utils.py:145-149).  Here each transform is a batched torch op over ``(n, C, W, H)`` on whatever
device the batch lives on:
  * deterministic part -- resize to (width, height) [identity at the configured 32x64], centre / random
    crop, patch masking, additive Gaussian noise: same arithmetic as the reference;
  * random photometric / geometric augmentation of the TRAIN transform (brightness+contrast jitter 0.1 with
    p 0.3, 5x5 Gaussian blur sigma in (0.01, 0.1) with p 0.5, rotation <= 3 degrees with p 0.5) --
    same distributions, drawn per image from torch's generator; not sample-identical to torchvision's RNG
    stream (no parity claim is made on augmented samples).

Camera pair (depth frames + segmentation masks; utils.py:12-128, 280-322, 422-454): ``define_img_transforms`` ->
(transform, mask_transform, eval_transform, sync_transform, sync_eval_transform), ``ImageTransform``, ``SyncTransform``,
``SyncEvalTransform``, ``SyncCenterReshapeTransform``, ``SyncRandomCrop``, ``SyncCenterCrop``.  Called on tensors they
are torch ops on any device; ``SyncTransform.fused`` builds a minibatch from the resident arenas in one native launch
(csrc/augment.h).  DESIGN.md section 4 has the parameter contract and the two evaluation-side deviations.

Tactile images in one launch (``offline_train.tactile_augment: "fused"``): ``define_tactile_augment`` -> (``TactileAugment``,
its ``train=False`` twin).  The train transform above with its random numbers apart from its arithmetic, image by image:
``draw`` on the CPU from the loader's generator (a window, a jitter and an angle per image, one noise seed per batch),
``apply`` in torch ops on any device, ``fused`` = draw + torch.ops.mi355ppo.tactile_augment, which builds the batch from the
resident arena in one native launch (csrc/tactile_augment.h).  It differs from the ``nn.Sequential`` in three recorded ways
(DESIGN.md section 4): a window per image instead of one per batch, the loader's generator instead of the device's, and
no 5-tap blur (sigma <= 0.1 moves no pixel by 1e-21 of the image's range).
"""
import math
import os
import random

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import draws, ops  # noqa: F401  (ops registers torch.ops.mi355ppo)


class GaussianNoise(nn.Module):
    """utils.py:457-466"""

    def __init__(self, std=0.1):
        super().__init__()
        self.std = std

    def forward(self, x):
        return x + torch.randn_like(x) * self.std if self.training else x


class Masking(nn.Module):
    """utils.py:191-216: zero whole patches with probability ``img_masking_prob`` (same mask for every
    channel of an image)."""

    def __init__(self, img_patch_size, img_masking_prob):
        super().__init__()
        self.img_patch_size, self.img_masking_prob = img_patch_size, img_masking_prob

    def forward(self, x):
        p = self.img_patch_size
        gh, gw = x.shape[-2] // p, x.shape[-1] // p
        drop = torch.rand((x.shape[0], gh, gw), device=x.device) < self.img_masking_prob
        return _mask_patches(x, ~drop, p)


class _Resize(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = tuple(size)

    def forward(self, x):
        if tuple(x.shape[-2:]) == self.size:
            return x
        return F.interpolate(x, size=self.size, mode='bilinear', align_corners=False, antialias=True)


class _Crop(nn.Module):
    def __init__(self, size, random_offset):
        super().__init__()
        self.size, self.random_offset = tuple(size), random_offset

    def forward(self, x):
        h, w = x.shape[-2:]
        ch, cw = self.size
        if (h, w) == (ch, cw):
            return x
        if self.random_offset and self.training:
            top = int(torch.randint(0, h - ch + 1, (1,)))
            left = int(torch.randint(0, w - cw + 1, (1,)))
        else:
            top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
        return x[..., top:top + ch, left:left + cw]


class _TrainAugment(nn.Module):
    """brightness/contrast jitter, 5x5 Gaussian blur, small rotation; each drawn per image."""

    def forward(self, x):
        if not self.training:
            return x
        n, dev = x.shape[0], x.device
        # ColorJitter(brightness=0.1, contrast=0.1), p = 0.3
        on = (torch.rand(n, 1, 1, 1, device=dev) < 0.3).to(x.dtype)
        b = 1 + (torch.rand(n, 1, 1, 1, device=dev) * 0.2 - 0.1) * on
        c = 1 + (torch.rand(n, 1, 1, 1, device=dev) * 0.2 - 0.1) * on
        x = (x * b).clamp(0, 1) * on + x * (1 - on)
        mean = x.mean(dim=(1, 2, 3), keepdim=True)
        x = ((x - mean) * c + mean).clamp(0, 1) * on + x * (1 - on)
        # GaussianBlur(5, sigma in (0.01, 0.1)), p = 0.5
        on = (torch.rand(n, device=dev) < 0.5)
        sigma = torch.rand(n, device=dev) * 0.09 + 0.01
        t = torch.arange(-2, 3, device=dev, dtype=x.dtype)
        k1 = torch.exp(-0.5 * (t[None, :] / sigma[:, None]) ** 2)
        k1 = k1 / k1.sum(1, keepdim=True)
        ident = torch.zeros(5, device=dev, dtype=x.dtype)
        ident[2] = 1
        k1 = torch.where(on[:, None], k1, ident[None, :])
        C = x.shape[1]
        xp = F.pad(x, (2, 2, 2, 2), mode='reflect').reshape(1, n * C, x.shape[2] + 4, x.shape[3] + 4)
        kh = k1.repeat_interleave(C, 0)
        xp = F.conv2d(xp, kh[:, None, :, None], groups=n * C)
        xp = F.conv2d(xp, kh[:, None, None, :], groups=n * C)
        x = xp.reshape(n, C, *x.shape[2:])
        # RandomRotation(3 degrees), p = 0.5 (nearest resampling, zero fill: torchvision's defaults)
        on = (torch.rand(n, device=dev) < 0.5).to(x.dtype)
        ang = (torch.rand(n, device=dev) * 6 - 3) * on * (math.pi / 180)
        cos, sin = torch.cos(ang), torch.sin(ang)
        H, W = x.shape[-2:]
        theta = torch.stack([torch.stack([cos, -sin * H / W, torch.zeros_like(cos)], 1),
                             torch.stack([sin * W / H, cos, torch.zeros_like(cos)], 1)], 1)
        grid = F.affine_grid(theta, list(x.shape), align_corners=False)
        return F.grid_sample(x, grid, mode='nearest', padding_mode='zeros', align_corners=False)


def define_tactile_transforms(width, height, crop_width, crop_height, img_patch_size=16, img_gaussian_noise=0.0,
                              img_masking_prob=0.0):
    """utils.py:219-277 -> (transform, eval_transform), both ``nn.Module``s over (n, C, W, H)."""
    stages = [_Resize((width, height)), _Crop((crop_width, crop_height), True), _TrainAugment()]
    if img_gaussian_noise > 0.0:
        stages.append(GaussianNoise(img_gaussian_noise))
    if img_masking_prob > 0.0:
        stages.append(Masking(img_patch_size, img_masking_prob))
    transform = nn.Sequential(*stages)
    eval_transform = nn.Sequential(_Resize((width, height)), _Crop((crop_width, crop_height), False))
    eval_transform.eval()
    return transform, eval_transform


# ---------------------------------------------------------------------------------------------
# camera pair: depth frames + segmentation masks (utils.py:12-128, 280-322, 422-454)
# ---------------------------------------------------------------------------------------------
def _center_offsets(h, w, ch, cw):
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))


def _center_crop(x, size):
    ch, cw = size
    h, w = x.shape[-2:]
    if (h, w) == (ch, cw):
        return x
    top, left = _center_offsets(h, w, ch, cw)
    return x[..., top:top + ch, left:left + cw]


# The draws and the torch-op steps SyncTransform, SyncEvalTransform and TactileAugment share.  Every draw is on the CPU from
# ``generator`` (torch's default when None); a stage that is off draws nothing, so a seeded run keeps its random stream.
def _draw_windows(n, size, crop, generator):
    """int32 (n, 2): (top, left) uniform over the valid positions; an axis with no room to move draws nothing."""
    offsets = torch.zeros(n, 2, dtype=torch.int32)
    for k in range(2):
        if size[k] > crop[k]:
            offsets[:, k] = torch.randint(0, size[k] - crop[k] + 1, (n,), generator=generator, dtype=torch.int32)
    return offsets


def _center_windows(n, size, crop):
    """int32 (n, 2): the centre window, n times."""
    return torch.tensor([_center_offsets(*size, *crop)], dtype=torch.int32).repeat(n, 1)


def _draw_keep(n, crop, patch, prob, generator):
    """uint8 (n, gh, gw), 0 with probability ``prob``: one grid of whole patches per image; None when ``prob`` is 0."""
    if not prob > 0.0:
        return None
    drop = torch.rand(n, crop[0] // patch, crop[1] // patch, generator=generator) < prob
    return (~drop).to(torch.uint8)


def _draw_seed(noise_std, generator):
    """One 63-bit noise seed per batch; 0, and nothing drawn, without noise."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator)) if noise_std > 0.0 else 0


def _gather_windows(x, offsets, crop):
    """(n, ..., H, W), one (top, left) per row of x -> (n, ..., ch, cw): every row's own window, one advanced index."""
    dev = x.device
    off = offsets.to(dev).long()
    ni = torch.arange(x.shape[0], device=dev)[:, None, None]
    ri = (off[:, :1] + torch.arange(crop[0], device=dev))[:, :, None]
    ci = (off[:, 1:] + torch.arange(crop[1], device=dev))[:, None, :]
    return x.movedim((-2, -1), (1, 2))[ni, ri, ci].movedim((1, 2), (-2, -1))


def _mask_patches(y, keep, patch):
    """(n, C, h, w) times ``keep`` (n, gh, gw), every entry a whole patch, the same for every channel; rows / columns past
    the last whole patch are kept.  A copy: ``y`` is left as it is."""
    gh, gw = keep.shape[1:]
    m = keep.to(y.device).to(y.dtype).repeat_interleave(patch, 1).repeat_interleave(patch, 2)
    y = y.clone()
    y[:, :, :gh * patch, :gw * patch] *= m.unsqueeze(1)
    return y


def _rotate(x, ang):
    """(n, C, H, W) rotated about the image centre by ``ang`` (n,) radians: nearest resampling, zero fill (torchvision's
    defaults) -- the arithmetic of ``_TrainAugment`` above, and the one csrc/aug_pixel.h restates per pixel."""
    cos, sin = torch.cos(ang), torch.sin(ang)
    H, W = x.shape[-2:]
    zero = torch.zeros_like(cos)
    theta = torch.stack([torch.stack([cos, -sin * H / W, zero], 1), torch.stack([sin * W / H, cos, zero], 1)], 1)
    grid = F.affine_grid(theta.to(x.dtype), list(x.shape), align_corners=False)
    return F.grid_sample(x, grid, mode='nearest', padding_mode='zeros', align_corners=False)


class _RandomRotation(nn.Module):
    """v2.RandomRotation(degrees): ONE angle per call, uniform in +-degrees, for every image of the tensor."""

    def __init__(self, degrees):
        super().__init__()
        self.degrees = float(degrees)

    def forward(self, x):
        if not self.training or self.degrees == 0.0:
            return x
        ang = (torch.rand(1) * 2 - 1) * (self.degrees * math.pi / 180)
        y = x.reshape(-1, *x.shape[-3:])
        return _rotate(y, ang.to(x.device).expand(y.shape[0])).reshape(x.shape)


class ImageTransform:
    """utils.py:70-82: (B, T, C, H, W) -> the transform over (B*T, C, H, W) -> (B, T, C, h, w)."""

    def __init__(self, image_transform=None):
        self.image_transform = image_transform

    def __call__(self, img_input):
        B, T, C, H, W = img_input.shape
        y = img_input.reshape(-1, C, H, W)
        if self.image_transform is not None:
            y = self.image_transform(y)
        return y.reshape(B, T, C, *y.shape[2:])


class SyncRandomCrop(nn.Module):
    """utils.py:422-443: one random window for the image and its mask; kept until ``reset()``."""

    def __init__(self, crop_size):
        super().__init__()
        self.crop_size = tuple(crop_size)
        self.crop_params = None

    def forward(self, img, mask):
        if self.crop_params is None:
            h, w = img.shape[-2:]
            ch, cw = self.crop_size
            if ch > h or cw > w:
                raise ValueError(f"crop size {self.crop_size} larger than the image {(h, w)}")
            i = int(torch.randint(0, h - ch + 1, (1,))) if h > ch else 0
            j = int(torch.randint(0, w - cw + 1, (1,))) if w > cw else 0
            self.crop_params = (i, j, ch, cw)
        i, j, ch, cw = self.crop_params
        return img[..., i:i + ch, j:j + cw], mask[..., i:i + ch, j:j + cw]

    def reset(self):
        self.crop_params = None


class SyncCenterCrop(nn.Module):
    """utils.py:446-454"""

    def __init__(self, crop_size):
        super().__init__()
        self.crop_size = tuple(crop_size)

    def forward(self, img, mask):
        return _center_crop(img, self.crop_size), _center_crop(mask, self.crop_size)


def _stage(transform, kind):
    if transform is None:
        return None
    return next((m for m in transform.modules() if isinstance(m, kind)), None)


class SyncTransform(nn.Module):
    """utils.py:85-106 with the reference's constructor: resize both, ONE random crop for the image and its mask, then
    each through its own chain (``img_transform``: rotation, noise, patch masking; ``mask_transform``: rotation, noise).

    The random numbers of a call are separated from the arithmetic:
      ``draw(B, T, generator)``  -> (offsets, angles, keep, seed) on the CPU, one crop window and one angle pair per
                                    sample (all its T frames), one patch mask per frame;
      ``apply(img, mask, ...)``  -> the transform of a (B, T, C, H, W) pair with those draws, in plain torch ops on any
                                    device (the noise is ``torch.randn``);
      ``fused(arena, arena, rows)`` -> draw + torch.ops.mi355ppo.image_pair_augment: the gather from the resident arenas
                                    and the whole transform in one launch (the noise is the kernel's counter hash of
                                    ``seed``);
      ``draw_seeded(B, T, seed)`` / ``apply_seeded`` / ``fused_seeded(arena2d, arena2d, rows, seed)`` -> the online
                                    student's form: no crop, either tensor may be absent, and every draw the counter hash
                                    of one seed, evaluated by the kernel itself
                                    (torch.ops.mi355ppo.image_pair_augment_seeded, csrc/augment_seeded.h);
                                    ``draw_seeded`` + ``apply_seeded`` is the same function in torch ops.
    ``forward(img, mask)`` is draw + apply from torch's default generator, on one item (T, C, H, W) as the dataset calls
    it, or on a batch."""

    def __init__(self, crop_size, downsample, img_transform, mask_transform):
        super().__init__()
        self.crop_size = tuple(crop_size)
        self.sync_crop = SyncRandomCrop(crop_size)
        self.downsample = downsample
        self.img_transform = img_transform
        self.mask_transform = mask_transform
        self.generator = None
        rot, noise, mask = (_stage(img_transform, k) for k in (_RandomRotation, GaussianNoise, Masking))
        self.rotation_deg = rot.degrees if rot is not None else 0.0
        self.noise_std = float(noise.std) if noise is not None else 0.0
        self.masking_prob = float(mask.img_masking_prob) if mask is not None else 0.0
        self.patch = int(mask.img_patch_size) if mask is not None else 1

    @property
    def size(self):
        """(rows, columns) the crop is taken from: the resize target."""
        return self.downsample.size

    @property
    def is_identity(self):
        return (self.crop_size == tuple(self.size) and self.rotation_deg == 0.0 and self.noise_std == 0.0
                and self.masking_prob == 0.0)

    def draw(self, B, T, generator=None):
        """The random numbers of one batch, from ``generator`` (torch's default when None), as CPU tensors: ``offsets``
        int32 (B, 2) uniform over the valid (top, left); ``angles`` fp32 (B, 2) radians uniform in +-rotation_deg, column
        0 the image's and column 1 the mask's; ``keep`` uint8 (B*T, gh, gw) or None; ``seed`` a 63-bit int (0 without
        noise).  A stage that is off draws nothing."""
        offsets = _draw_windows(B, self.size, self.crop_size, generator)
        angles = torch.zeros(B, 2)
        if self.rotation_deg > 0.0:
            angles = (torch.rand(B, 2, generator=generator) * 2 - 1) * (self.rotation_deg * math.pi / 180)
        keep = _draw_keep(B * T, self.crop_size, self.patch, self.masking_prob, generator)
        return offsets, angles, keep, _draw_seed(self.noise_std, generator)

    def apply(self, img, mask, offsets, angles, keep=None, noise_std=0.0):
        """(B, T, C, H, W) pair at the resize target -> cropped, rotated, noised, masked pair: batched torch ops."""
        return self._apply(img, mask, offsets, angles, keep, noise_std, lambda k, y: torch.randn_like(y) * noise_std)

    def _apply(self, img, mask, offsets, angles, keep, noise_std, noise_of):
        """``apply`` with the noise term of tensor ``k`` (0 = image, 1 = mask) from ``noise_of(k, y)``; a tensor that is None
        stays None."""
        ch, cw = self.crop_size
        turned = (angles != 0).any(0).tolist()            # on the draw's (CPU) tensor: no device read-back
        outs = []
        for k, x in enumerate((img, mask)):
            if x is None:
                outs.append(None)
                continue
            B, T, C = x.shape[:3]
            y = _gather_windows(x, offsets, self.crop_size).reshape(B * T, C, ch, cw)
            if turned[k]:
                y = _rotate(y, angles[:, k].to(x.device).repeat_interleave(T))
            if noise_std > 0.0:
                y = y + noise_of(k, y)
            if k == 0 and keep is not None:
                y = _mask_patches(y, keep, self.patch)
            outs.append(y.reshape(B, T, C, ch, cw))
        return outs[0], outs[1]

    @property
    def max_rad(self):
        """``rotation_deg`` in radians, formed in double and rounded once to fp32: the value the seeded kernel is handed."""
        return float(np.float32(self.rotation_deg * math.pi / 180))

    def draw_seeded(self, B, T, seed):
        """The tuple ``draw`` returns, as k_image_pair_augment_seeded draws it from ``seed`` alone (the table of
        csrc/augment_seeded.h, restated on the CPU through ``draws``): ``offsets`` 0 (no crop online); the angle of
        (sample b, tensor which) is the hash of element ``2 b + which`` -- float64 arithmetic on exact operands rounded once
        to fp32, the kernel's bits; ``keep`` cell by cell at element ``(b T + t) gh gw + cell``; the returned seed is
        ``seed``, which the noise hashes too.  No generator is asked for anything; a stage that is off evaluates no hash."""
        B, T, seed = int(B), int(T), int(seed)
        angles = torch.zeros(B, 2)
        if self.rotation_deg > 0.0:
            unit = draws.unit(draws.tok_hash(seed, draws.SITES["IMG_SITE_ANGLE"], torch.arange(2 * B)))
            angles = (unit * self.max_rad).float().reshape(B, 2)
        gh, gw = self.crop_size[0] // self.patch, self.crop_size[1] // self.patch
        keep = None
        if self.masking_prob > 0.0 and gh * gw > 0:
            keep = draws.keep_grid(seed, draws.SITES["IMG_SITE_KEEP"], self.masking_prob, (B * T, gh, gw))
        return torch.zeros(B, 2, dtype=torch.int32), angles, keep, seed

    def apply_seeded(self, img, mask, offsets, angles, keep=None, noise_std=0.0, seed=0):
        """``apply`` with the noise the kernels add: ``draws.gauss`` of ``seed`` on plane 0 (image) and plane 1 (mask), at
        every element's linear index in its output, times ``noise_std`` rounded to fp32 (the kernel is handed a float).  Any
        device and float dtype; either tensor may be None."""
        std = float(np.float32(noise_std))
        return self._apply(img, mask, offsets, angles, keep, noise_std,
                           lambda k, y: std * draws.gauss(int(seed), k, draws.elements(y.shape, y.device), y.dtype))

    def fused_seeded(self, img_arena2d, seg_arena2d, rows, seed, want_draws=False):
        """The online student's minibatch in one native launch, every draw hashed from ``seed``: the arenas are the rollout
        storage's time-major camera fields as the gather sees them, (horizon * envs, T * H * W) single-channel frames at
        ``size``, read in place (either may be None); ``rows`` the minibatch's int64 flat rows on their device ->
        (img, seg, draws): fp32 (B, T, 1, H, W) where the arena is there and, with ``want_draws``, int32 (B, 2), the bits of
        the kernel's own angles (else None).  There is no crop online.  Above the kernel's limits the same draws go through
        ``apply_seeded``."""
        H, W = (int(v) for v in self.size)
        if self.crop_size != (H, W):
            raise NotImplementedError(f"SyncTransform.fused_seeded does not crop: crop size {self.crop_size}, stored {(H, W)}")
        arenas = [a for a in (img_arena2d, seg_arena2d) if a is not None]
        if not arenas:
            raise ValueError("img_arena2d / seg_arena2d: expected at least one arena, got None for both")
        for a in arenas:
            if a.dim() != 2 or a.shape[1] % (H * W) != 0 or a.shape[1] == 0 or a.shape != arenas[0].shape:
                raise ValueError(f"arena2d: expected (rows, T * {H} * {W}), the same for both, got {tuple(a.shape)}")
        T, B = arenas[0].shape[1] // (H * W), rows.numel()
        gather = lambda a: None if a is None else a.index_select(0, rows).reshape(B, T, 1, H, W)   # noqa: E731
        if not self.training:
            return gather(img_arena2d), gather(seg_arena2d), None
        cells = (H // self.patch) * (W // self.patch) if self.masking_prob > 0.0 else 0
        if cells > ops.IMG_AUG_MAX_CELLS or H * W > 1 << 24:   # beyond the kernel: the same draws in torch ops
            offsets, angles, keep, seed = self.draw_seeded(B, T, seed)
            img, seg = self.apply_seeded(gather(img_arena2d), gather(seg_arena2d), offsets, angles, keep, self.noise_std, seed)
            return img, seg, (angles.view(torch.int32).to(rows.device) if want_draws else None)
        return torch.ops.mi355ppo.image_pair_augment_seeded(img_arena2d, seg_arena2d, rows, T, H, W, self.patch, self.noise_std,
                                                            self.masking_prob, self.max_rad, int(seed), bool(want_draws))

    def forward(self, img, mask):
        item = img.dim() == 4
        if item:
            img, mask = img[None], mask[None]
        B, T, C = img.shape[:3]
        img = self.downsample(img.reshape(-1, *img.shape[2:])).reshape(B, T, C, *self.size)
        mask = self.downsample(mask.reshape(-1, *mask.shape[2:])).reshape(B, T, C, *self.size)
        offsets, angles, keep, _ = self.draw(B, T, self.generator)
        img, mask = self.apply(img, mask, offsets, angles, keep, self.noise_std if self.training else 0.0)
        return (img[0], mask[0]) if item else (img, mask)

    def _pair_op(self, img_arena, seg_arena, rows, offsets, angles, keep, noise_std, seed):
        if tuple(img_arena.shape[-2:]) != tuple(self.size):
            # stored at another size: resize the gathered batch, then the op reads it row by row
            B, T, C = rows.numel(), img_arena.shape[1], img_arena.shape[2]
            img_arena, seg_arena = (self.downsample(a.index_select(0, rows).reshape(B * T, C, *a.shape[-2:]))
                                    .reshape(B, T, C, *self.size).contiguous() for a in (img_arena, seg_arena))
            rows = torch.arange(B, device=rows.device)
        dev = img_arena.device
        return torch.ops.mi355ppo.image_pair_augment(
            img_arena, seg_arena, rows, offsets.to(dev), angles.to(dev),
            keep.to(dev) if keep is not None else None, self.crop_size[0], self.crop_size[1],
            self.patch, noise_std, seed)

    def fused(self, img_arena, seg_arena, rows, generator=None):
        """``(arena.index_select(0, rows) for both) -> forward`` as one native launch: the arenas are the loader's resident
        (N, T, 1, H, W) fields, ``rows`` the batch's int64 sample numbers on their device."""
        offsets, angles, keep, seed = self.draw(rows.numel(), img_arena.shape[1],
                                                generator if generator is not None else self.generator)
        return self._pair_op(img_arena, seg_arena, rows, offsets, angles, keep, self.noise_std, seed)


class SyncEvalTransform(SyncTransform):
    """utils.py:109-128, deterministic: resize, centre crop, nothing random.  (The reference sends the mask through the
    TRAIN-time ``mask_transform`` here -- a random rotation at validation -- and resizes the cropped pair a second time;
    neither is copied: DESIGN.md.)  Same constructor; ``fused`` is the centre-crop gather in one launch."""

    @property
    def is_identity(self):
        return self.crop_size == tuple(self.size)

    def draw(self, B, T, generator=None):
        return _center_windows(B, self.size, self.crop_size), torch.zeros(B, 2), None, 0

    def forward(self, img, mask):
        lead = img.shape[:-3]
        img = self.downsample(img.reshape(-1, *img.shape[-3:]))
        mask = self.downsample(mask.reshape(-1, *mask.shape[-3:]))
        img, mask = _center_crop(img, self.crop_size), _center_crop(mask, self.crop_size)
        return img.reshape(*lead, *img.shape[-3:]), mask.reshape(*lead, *mask.shape[-3:])

    def fused(self, img_arena, seg_arena, rows, generator=None):
        offsets, angles, _, _ = self.draw(rows.numel(), img_arena.shape[1])
        return self._pair_op(img_arena, seg_arena, rows, offsets, angles, None, 0.0, 0)


class SyncCenterReshapeTransform(nn.Module):
    """utils.py:12-37: (B, T, C, H, W) pair -> centre crop to ``crop_size`` -> each through its transform (None = none)."""

    def __init__(self, crop_size, img_transform, mask_transform):
        super().__init__()
        self.crop_size = tuple(crop_size)
        self.img_transform, self.mask_transform = img_transform, mask_transform

    def forward(self, img, mask):
        B, T, C, H, W = img.shape
        img = _center_crop(img.reshape(-1, C, H, W), self.crop_size)
        mask = _center_crop(mask.reshape(-1, C, H, W), self.crop_size)
        if self.img_transform is not None:
            img = self.img_transform(img)
        if self.mask_transform is not None:
            mask = self.mask_transform(mask)
        return img.reshape(B, T, C, *img.shape[2:]), mask.reshape(B, T, C, *mask.shape[2:])


def define_img_transforms(width, height, crop_width, crop_height, img_patch_size=16, img_gaussian_noise=0.0,
                          img_masking_prob=0.0, rotation_deg=0.0):
    """utils.py:280-322 -> (transform, mask_transform, eval_transform, sync_transform, sync_eval_transform).  The
    reference hard-codes ``RandomRotation(degrees=1)`` in both chains; here it is ``rotation_deg`` (0 = no rotation
    stage), so a run that never rotated keeps its random stream."""
    downsample = _Resize((width, height))
    chain, mask_chain = [], []
    if rotation_deg > 0.0:
        chain.append(_RandomRotation(rotation_deg))
        mask_chain.append(_RandomRotation(rotation_deg))
    if img_gaussian_noise > 0.0:
        chain.append(GaussianNoise(img_gaussian_noise))
        mask_chain.append(GaussianNoise(img_gaussian_noise))
    if img_masking_prob > 0.0:
        chain.append(Masking(img_patch_size, img_masking_prob))
    transform, mask_transform = nn.Sequential(*chain), nn.Sequential(*mask_chain)
    eval_transform = nn.Sequential(downsample, _Crop((crop_width, crop_height), False))
    eval_transform.eval()
    sync_transform = SyncTransform((crop_width, crop_height), downsample, transform, mask_transform)
    sync_eval_transform = SyncEvalTransform((crop_width, crop_height), downsample, eval_transform, mask_transform)
    return transform, mask_transform, eval_transform, sync_transform, sync_eval_transform


class TactileTransform:
    """utils.py:131-156: (B, T, fingers, C, H, W) -> transformed, same rank.  One batched call instead
    of the reference's per-image loop."""

    def __init__(self, tactile_transform=None):
        self.tactile_transform = tactile_transform

    def __call__(self, tac_input):
        B, T, Fg, C, H, W = tac_input.shape
        y = tac_input.reshape(-1, C, H, W)
        if self.tactile_transform is not None:
            y = self.tactile_transform(y)
        return y.reshape(B, T, Fg, C, *y.shape[2:])


# ---------------------------------------------------------------------------------------------
# tactile images, random numbers apart from the arithmetic: one native launch per batch (csrc/tactile_augment.h)
# ---------------------------------------------------------------------------------------------
class TactileAugment(nn.Module):
    """The train transform of ``define_tactile_transforms`` -- crop, brightness / contrast jitter (p 0.3), rotation
    <= 3 degrees (p 0.5), Gaussian noise, patch masking -- with the random numbers of a call apart from its arithmetic,
    image by image: an image is one single-channel (sample, t, finger) plane and has its own window, jitter, angle and
    patch mask.  ``_TrainAugment``'s 5-tap blur (sigma <= 0.1) is left out: it moves no pixel by 1e-21 of the image's
    range.
      ``draw(n_images, generator)`` -> (offsets, jitter, angles, keep, seed) on the CPU;
      ``apply(x, ...)``             -> the transform of (..., C, H, W) images with those draws, in plain torch ops on any
                                       device and in x's dtype; the noise is the kernel's counter hash of ``seed``;
      ``fused(arena, rows)``        -> draw + torch.ops.mi355ppo.tactile_augment: the gather from the resident
                                       (N, T, F, 1, H, W) arena and the whole transform in one launch;
      ``draw_seeded(n_images, seed)`` / ``fused_seeded(arena2d, rows, seed)`` -> the online student's form: no crop, and
                                       every draw the counter hash of one seed, evaluated by the kernel itself
                                       (torch.ops.mi355ppo.tactile_augment_seeded); ``draw_seeded`` + ``apply`` is the same
                                       function in torch ops.
    ``forward(x)`` is draw + apply from torch's default CPU generator.  In ``eval()`` mode (``train=False``) it is the
    eval transform: the centre window, nothing random, nothing drawn."""

    JITTER_P, ROTATE_P, JITTER, ROTATE_DEG = 0.3, 0.5, 0.1, 3.0

    def __init__(self, size, crop_size, patch=16, noise_std=0.0, masking_prob=0.0, train=True):
        super().__init__()
        self._size, self.crop_size = tuple(size), tuple(crop_size)
        if self.crop_size[0] > self._size[0] or self.crop_size[1] > self._size[1]:
            raise ValueError(f"crop size {self.crop_size} larger than the image {self._size}")
        self.patch, self.noise_std, self.masking_prob = int(patch), float(noise_std), float(masking_prob)
        self.generator = None
        self.train(bool(train))

    @property
    def size(self):
        """(rows, columns) the crop is taken from."""
        return self._size

    @property
    def is_identity(self):
        return not self.training and self.crop_size == self._size

    def draw(self, n_images, generator=None):
        """The random numbers of one batch, from ``generator`` (torch's default when None), as CPU tensors, one row per
        image: ``offsets`` int32 (n, 2) uniform over the valid (top, left); ``jitter`` fp32 (n, 3) = (flag, brightness,
        contrast), the factors uniform in 1 +- 0.1 where the flag is 1 and 1 elsewhere; ``angles`` fp32 (n,) radians,
        uniform in +- 3 degrees with probability 0.5 and 0 elsewhere; ``keep`` uint8 (n, gh, gw) or None; ``seed`` one
        63-bit int per batch (0 without noise).  A stage that is off draws nothing; evaluation draws nothing at all."""
        n = int(n_images)
        jitter = torch.ones(n, 3)
        jitter[:, 0] = 0
        angles = torch.zeros(n)
        if not self.training:
            return _center_windows(n, self._size, self.crop_size), jitter, angles, None, 0
        offsets = _draw_windows(n, self._size, self.crop_size, generator)
        u = torch.rand(3, n, generator=generator)
        on = u[0] < self.JITTER_P
        jitter[:, 0] = on.float()
        jitter[:, 1] = torch.where(on, 1 + (u[1] * 2 - 1) * self.JITTER, jitter[:, 1])
        jitter[:, 2] = torch.where(on, 1 + (u[2] * 2 - 1) * self.JITTER, jitter[:, 2])
        u = torch.rand(2, n, generator=generator)
        angles = torch.where(u[0] < self.ROTATE_P, (u[1] * 2 - 1) * (self.ROTATE_DEG * math.pi / 180), angles)
        keep = _draw_keep(n, self.crop_size, self.patch, self.masking_prob, generator)
        return offsets, jitter, angles, keep, _draw_seed(self.noise_std, generator)

    def draw_seeded(self, n_images, seed):
        """The tuple ``draw`` returns, as k_tactile_augment_seeded draws it from ``seed`` alone (the table of
        csrc/tactile_augment_seeded.h, restated on the CPU through ``draws``): ``offsets`` 0 (no crop online); image
        i's flags are the integer comparisons of its hashes; its factors and angle are float64 arithmetic on exact operands
        rounded once to fp32 -- the kernel's bits; ``keep`` cell by cell at element ``i * gh * gw + cell``; the returned
        seed is ``seed``, which the noise hashes too.  Evaluation draws nothing."""
        n, seed = int(n_images), int(seed)
        if not self.training:
            return self.draw(n)
        img = torch.arange(n)
        h = {k: draws.tok_hash(seed, draws.SITES["TAC_SITE_" + k], img)
             for k in ("JITTER", "BRIGHT", "CONTRAST", "ROTATE", "ANGLE")}
        on, turn = h["JITTER"] < draws.threshold(self.JITTER_P), h["ROTATE"] < draws.threshold(self.ROTATE_P)
        amp, rad = float(np.float32(self.JITTER)), float(np.float32(self.ROTATE_DEG * math.pi / 180))
        one = torch.ones(n)
        jitter = torch.stack([on.float(), torch.where(on, (draws.unit(h["BRIGHT"]) * amp + 1.0).float(), one),
                              torch.where(on, (draws.unit(h["CONTRAST"]) * amp + 1.0).float(), one)], 1)
        angles = torch.where(turn, (draws.unit(h["ANGLE"]) * rad).float(), torch.zeros(n))
        gh, gw = self.crop_size[0] // self.patch, self.crop_size[1] // self.patch
        keep = None
        if self.masking_prob > 0.0 and gh * gw > 0:
            keep = draws.keep_grid(seed, draws.SITES["TAC_SITE_KEEP"], self.masking_prob, (n, gh, gw))
        return torch.zeros(n, 2, dtype=torch.int32), jitter, angles, keep, seed

    @staticmethod
    def pack(offsets, jitter, angles):
        """The draws of ``draw`` as the op's ``params``: int32 (n, 6) = top, left, flag, bits of (b, c, angle)."""
        return torch.cat([offsets.to(torch.int32), (jitter[:, :1] != 0).to(torch.int32),
                          jitter[:, 1:].float().contiguous().view(torch.int32),
                          angles.float().reshape(-1, 1).view(torch.int32)], 1)

    def apply(self, x, offsets, jitter, angles, keep=None, noise_std=0.0, seed=0):
        """(..., C, H, W) images at ``size``, one row of the draws per image -> (..., C, ch, cw): batched torch ops."""
        lead, (C, H, W) = x.shape[:-3], x.shape[-3:]
        ch, cw = self.crop_size
        dev = x.device
        y = x.reshape(-1, C, H, W)
        n = y.shape[0]
        if (H, W) != (ch, cw):
            y = _gather_windows(y, offsets, self.crop_size)
        if bool((jitter[:, 0] != 0).any()):               # on the draw's (CPU) tensor: no device read-back
            j = jitter.to(dev).to(y.dtype)
            on, b, c = (j[:, k].reshape(n, 1, 1, 1) for k in range(3))
            z = (y * b).clamp(0, 1)
            mean = z.mean(dim=(1, 2, 3), keepdim=True)
            y = torch.where(on != 0, ((z - mean) * c + mean).clamp(0, 1), y)
        if bool((angles != 0).any()):
            ang = angles.to(dev)
            y = torch.where((ang != 0).reshape(n, 1, 1, 1), _rotate(y.contiguous(), ang), y)
        if noise_std > 0.0:
            z = draws.gauss(int(seed), draws.PLANES["TAC_NOISE_PLANE"], draws.elements(y.shape, dev), y.dtype)
            y = y + float(np.float32(noise_std)) * z
        if keep is not None:
            y = _mask_patches(y, keep, self.patch)
        return y.reshape(*lead, C, ch, cw)

    def forward(self, x):
        offsets, jitter, angles, keep, seed = self.draw(x.numel() // math.prod(x.shape[-3:]), self.generator)
        return self.apply(x, offsets, jitter, angles, keep, self.noise_std if self.training else 0.0, seed)

    def check_arena(self, arena):
        """The fused path reads single-channel frames stored at ``size``; anything else is the torch path's."""
        if arena.dim() != 6 or arena.shape[3] != 1:
            raise NotImplementedError(f"offline_train.tactile_augment: 'fused' reads single-channel (gray) tactile frames, "
                                      f"got an arena of shape {tuple(arena.shape)}; use 'torch'")
        if tuple(arena.shape[-2:]) != self._size:
            raise NotImplementedError(f"offline_train.tactile_augment: 'fused' does not resize: the frames are stored at "
                                      f"{tuple(arena.shape[-2:])}, tactile_width x tactile_height is {self._size}; use 'torch'")

    def fused_seeded(self, arena2d, rows, seed, want_draws=False, fingers=3):
        """The online student's minibatch in one native launch, every draw hashed from ``seed``: ``arena2d`` the rollout
        storage's time-major tactile arena as the gather sees it, (horizon * envs, history * fingers * H * W) single-channel
        frames at ``size``, read in place; ``rows`` the minibatch's int64 flat rows on its device -> (out, draws): fp32
        (B, history, fingers, 1, H, W) and, with ``want_draws``, the kernel's own draws as ``pack`` lays them out (else None).
        There is no crop online.  Above the kernel's window the same draws go through ``apply``."""
        H, W = self._size
        if self.crop_size != self._size:
            raise NotImplementedError(f"TactileAugment.fused_seeded does not crop: crop size {self.crop_size}, stored {self._size}")
        if arena2d.dim() != 2 or arena2d.shape[1] % (fingers * H * W) != 0 or arena2d.shape[1] == 0:
            raise ValueError(f"arena2d: expected (rows, history * {fingers} * {H} * {W}), got {tuple(arena2d.shape)}")
        arena = arena2d.reshape(arena2d.shape[0], -1, fingers, 1, H, W)
        if not self.training:
            return arena.index_select(0, rows), None
        if H * W > ops.TACTILE_AUG_MAX_PIXELS:            # larger than the kernel's window: the same draws in torch ops
            n = rows.numel() * arena.shape[1] * fingers
            offsets, jitter, angles, keep, seed = self.draw_seeded(n, seed)
            out = self.apply(arena.index_select(0, rows), offsets, jitter, angles, keep, self.noise_std, seed)
            return out, (self.pack(offsets, jitter, angles).to(arena.device) if want_draws else None)
        return torch.ops.mi355ppo.tactile_augment_seeded(arena, rows, H, W, self.patch, self.noise_std, self.masking_prob,
                                                         int(seed), bool(want_draws))

    def fused(self, arena, rows, generator=None):
        """``arena.index_select(0, rows) -> forward`` as one native launch: ``arena`` the loader's resident
        (N, T, F, 1, H, W) field, ``rows`` the batch's int64 sample numbers on its device.  Every draw of the batch
        crosses to the device in ONE copy."""
        self.check_arena(arena)
        n = rows.numel() * arena.shape[1] * arena.shape[2]
        offsets, jitter, angles, keep, seed = self.draw(n, generator if generator is not None else self.generator)
        noise_std = self.noise_std if self.training else 0.0
        ch, cw = self.crop_size
        if ch * cw > ops.TACTILE_AUG_MAX_PIXELS:          # larger than the kernel's window: the same draws in torch ops
            return self.apply(arena.index_select(0, rows), offsets, jitter, angles, keep, noise_std, seed)
        words = self.pack(offsets, jitter, angles)
        if keep is None:
            params, keep_d = words.to(arena.device), None
        else:
            both = torch.cat([words.view(torch.uint8).reshape(-1), keep.reshape(-1)]).to(arena.device)
            params = both[:words.numel() * 4].view(torch.int32).view(n, ops.TACTILE_AUG_WORDS)
            keep_d = both[words.numel() * 4:].view(keep.shape)
        return torch.ops.mi355ppo.tactile_augment(arena, rows, params, keep_d, ch, cw, self.patch, noise_std, seed)


def define_tactile_augment(width, height, crop_width, crop_height, img_patch_size=16, img_gaussian_noise=0.0,
                           img_masking_prob=0.0):
    """``define_tactile_transforms``' arguments -> (TactileAugment, its ``train=False`` twin)."""
    args = ((width, height), (crop_width, crop_height), img_patch_size)
    return (TactileAugment(*args, img_gaussian_noise, img_masking_prob, train=True),
            TactileAugment(*args, 0.0, 0.0, train=False))


def set_seed(seed, torch_deterministic=False, rank=0):
    """utils.py:159-189"""
    if seed == -1 and torch_deterministic:
        seed = 42 + rank
    elif seed == -1:
        seed = np.random.randint(0, 10000)
    else:
        seed = seed + rank
    print("Setting seed: {}".format(seed))
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def log_output(*args, **kwargs):
    """utils.py:648-678 renders diagnostic figures of a batch; plotting is outside the scope table
     -- kept as a callable no-op so ``Runner.train`` keeps its call sites."""
    return None
