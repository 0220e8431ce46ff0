"""Point-cloud augmentation applied by the environment before the PointNet sees the cloud
(isaacgyminsertion/tasks/factory_tactile/factory_utils.py:83-165: ``PointCloudAugmentations``): same method
names and argument meaning; every method is batched elementwise torch on the device the cloud lives on, so it
adds a handful of launches per environment step to the rollout, nothing to the update.  ``augment`` applies what
the reference applies (point-wise + per-env constant noise; rotation / outliers / dropout exist but are commented
out there, factory_utils.py:156-162).

``PclAugment`` is the learner-side form of the same augmentation: the whole chain, with the environment's per-step hit and
per-episode parameters, in one native launch (csrc/pcl_augment.h)."""
import math

import numpy as np
import torch

from .. import draws


class PointCloudAugmentations:
    def __init__(self, num_points=400, sigma=0.001, noise_clip=0.001, rotate_range=(-10, 10), scale_range=(0.8, 1.2),
                 dropout_ratio=0.2):
        self.num_points, self.sigma, self.noise_clip = num_points, sigma, noise_clip
        self.const_noise = 0.001
        self.rotate_range, self.scale_range, self.dropout_ratio = rotate_range, scale_range, dropout_ratio

    def random_noise(self, pointcloud_batch, pcl_noise, noise_prob=0.3):
        """clipped N(0, sigma) on a random 30 % of the points + a clipped per-env offset (in place, like the
        reference: factory_utils.py:94-101)."""
        B, N, _ = pointcloud_batch.shape
        jitter = (torch.randn_like(pointcloud_batch) * self.sigma).clamp_(-self.noise_clip, self.noise_clip)
        hit = (torch.rand(B, N, 1, device=pointcloud_batch.device) < noise_prob).to(pointcloud_batch.dtype)
        pointcloud_batch += jitter * hit
        return pointcloud_batch + (pcl_noise * self.const_noise).clamp(-self.noise_clip, self.noise_clip)

    def random_rotate(self, pointcloud_batch, angles_rad, axes):
        """row-vector points times the axis rotation of each env (axes: 0 = x, 1 = y, 2 = z)."""
        c, s = torch.cos(angles_rad), torch.sin(angles_rad)
        o, z = torch.ones_like(c), torch.zeros_like(c)
        rx = torch.stack([o, z, z, z, c, -s, z, s, c], -1)
        ry = torch.stack([c, z, s, z, o, z, -s, z, c], -1)
        rz = torch.stack([c, -s, z, s, c, z, z, z, o], -1)
        sel = axes.reshape(-1, 1)
        rot = torch.where(sel == 0, rx, torch.where(sel == 1, ry, torch.where(sel == 2, rz, torch.eye(
            3, device=c.device, dtype=c.dtype).reshape(1, 9).expand_as(rx))))
        return torch.bmm(pointcloud_batch, rot.reshape(-1, 3, 3))

    def random_scale_anisotropic(self, pointcloud_batch):
        lo, hi = self.scale_range
        f = torch.rand(pointcloud_batch.shape[0], 1, 3, device=pointcloud_batch.device) * (hi - lo) + lo
        return pointcloud_batch * f

    def add_outliers(self, pointcloud_batch, outlier_ratio=0.1, contour_prob=0.75, scale_factor=1.5):
        """replace a random 10 % of the points: 75 % just outside the cloud's bounding box, the rest N(0, 1.5)."""
        B, N, _ = pointcloud_batch.shape
        k, dev = int(N * outlier_ratio), pointcloud_batch.device
        lo = pointcloud_batch.min(dim=1, keepdim=True).values
        hi = pointcloud_batch.max(dim=1, keepdim=True).values
        beyond = torch.randn(B, k, 3, device=dev).abs()
        contour = torch.where(torch.rand(B, k, 3, device=dev) < 0.5, hi + beyond, lo - beyond)
        free = torch.randn(B, k, 3, device=dev) * scale_factor
        new = torch.where((torch.rand(B, k, 1, device=dev) < contour_prob), contour, free)
        idx = torch.randint(0, N, (B, k, 1), device=dev).expand(-1, -1, 3)
        return pointcloud_batch.scatter_(1, idx, new)

    def batch_random_dropout(self, coords, dropout_ratio=0.2, no_dropout_prob=0.8):
        """zero a random subset of points in the 20 % of clouds that are selected for dropout."""
        B, N, _ = coords.shape
        dev = coords.device
        if isinstance(dropout_ratio, float):
            ratios = torch.full((B, 1), dropout_ratio, device=dev)
        else:
            ratios = torch.rand(B, 1, device=dev) * (dropout_ratio[1] - dropout_ratio[0]) + dropout_ratio[0]
        exempt = torch.rand(B, 1, device=dev) >= 1 - no_dropout_prob
        drop = (torch.rand(B, N, device=dev) < ratios) & ~exempt
        return torch.where(drop.unsqueeze(-1), torch.zeros_like(coords), coords)

    def augment(self, pointcloud_batch, angle, axes, pcl_noise, dropout_ratio=0.2):
        if not pointcloud_batch.shape[0]:
            return pointcloud_batch
        return self.random_noise(pointcloud_batch, pcl_noise)


# ---------------------------------------------------------------------------------------------
# the same augmentation on the learner's side: one native launch per environment step (csrc/pcl_augment.h)
# ---------------------------------------------------------------------------------------------
class PclAugment:
    """``PointCloudAugmentations.augment`` with the reference's environment logic around it (factory_task_insertion.py:
    299-303, 876-881, 951-986: applied to ``hit_prob`` of the envs per step, with a per-episode offset / angle / axis), for
    the whole cloud tensor of an environment step -- ``points`` the 1..4 consecutive objects of the PointNets' layout -- and
    with the random numbers of a call apart from its arithmetic: every draw is the counter hash of csrc/pcl_augment.h (``draws``).
      ``draw()``                           -> the step's seed, from this object's private CPU generator;
      ``apply(clouds, episode, seed_step)`` -> the augmentation in plain torch ops, on any device and in clouds' dtype;
      ``fused(clouds, episode)``            -> draw + torch.ops.mi355ppo.pcl_augment: one launch.
    ``episode`` is the caller's int32 (N,) episode counter; the per-episode parameters change when it does.  Stages:
    noise (always), rotation (``rot_deg`` > 0), outliers (``outlier_ratio`` > 0), dropout (``dropout_ratio`` > 0).  The
    input is never written."""

    def __init__(self, points, hit_prob=0.7, rot_deg=0.0, outlier_ratio=0.0, dropout_ratio=0.0, sigma=0.001,
                 noise_clip=0.001, const_noise=0.001, noise_prob=0.3, contour_prob=0.75, outlier_scale=1.5,
                 no_dropout_prob=0.8, seed=0):
        self.points = [int(p) for p in points]
        if not 1 <= len(self.points) <= 4 or min(self.points) < 1:
            raise ValueError(f"points: expected 1..4 objects of at least one point, got {list(points)}")
        self.hit_prob, self.rot_deg, self.outlier_ratio = float(hit_prob), float(rot_deg), float(outlier_ratio)
        self.dropout_ratio, self.sigma, self.noise_clip = float(dropout_ratio), float(sigma), float(noise_clip)
        self.const_noise, self.noise_prob, self.contour_prob = float(const_noise), float(noise_prob), float(contour_prob)
        self.outlier_scale, self.no_dropout_prob = float(outlier_scale), float(no_dropout_prob)
        for nm in ("hit_prob", "outlier_ratio", "dropout_ratio", "noise_prob", "contour_prob", "no_dropout_prob"):
            if not 0 <= getattr(self, nm) <= 1:
                raise ValueError(f"{nm}: expected a value in [0, 1], got {getattr(self, nm)}")
        for nm in ("rot_deg", "sigma", "noise_clip"):
            if not getattr(self, nm) >= 0:
                raise ValueError(f"{nm}: expected >= 0, got {getattr(self, nm)}")
        self.generator = torch.Generator().manual_seed(int(seed))
        self.seed_episode = self.draw()
        self.seed_step = None            # the last seed ``fused`` drew

    def params(self):
        """The op's ``params`` (ops.PCL_AUG_PARAMS)."""
        return [self.sigma, self.noise_clip, self.const_noise, self.noise_prob, self.hit_prob, self.rot_deg,
                self.outlier_ratio, self.contour_prob, self.outlier_scale, self.dropout_ratio, self.no_dropout_prob]

    def draw(self):
        """One 63-bit seed from the private generator; torch's global generators are not touched."""
        return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=self.generator))

    def apply(self, clouds, episode, seed_step):
        pts, Pt = self.points, sum(self.points)
        N = clouds.shape[0]
        if clouds.numel() != N * Pt * 3:
            raise ValueError(f"clouds: expected {Pt * 3} coordinates per env for points {pts}, got {tuple(clouds.shape)}")
        x = clouds.reshape(N, Pt, 3)
        dt, dev = x.dtype, x.device

        def H(site, idx, seed=int(seed_step)):
            return draws.tok_hash(seed, draws.SITES["PCL_SITE_" + site], idx)

        def Z(plane, idx, seed=int(seed_step)):              # float64, then rounded once to the cloud's dtype
            return draws.gauss(seed, draws.PLANES["PCL_PLANE_" + plane], idx, torch.float64).to(dt)

        thr = draws.threshold
        f32 = lambda v: float(np.float32(v))   # noqa: E731  (the kernel receives fp32 scalars)
        ep = episode.detach().to(device=dev, dtype=torch.int64)
        se = (self.seed_episode, (self.seed_episode >> 32) + ep)                            # se = seed + (episode << 32)
        env = torch.arange(N, device=dev)
        g = env[:, None] * Pt + torch.arange(Pt, device=dev)[None]                          # (N, Pt) point numbers
        e = g[:, :, None] * 3 + torch.arange(3, device=dev)                                 # (N, Pt, 3)
        hit = H("HIT", env) < thr(self.hit_prob)
        clip = f32(self.noise_clip)
        # a. noise
        y = x
        jit = torch.zeros_like(x)
        if self.sigma > 0:
            mask = H("MASK", g) < thr(self.noise_prob)
            jit = (Z("JITTER", e) * f32(self.sigma)).clamp(-clip, clip) * mask.to(dt)[:, :, None]
        y = y + jit
        pn = Z("PN", env[:, None] * 3 + torch.arange(3, device=dev), (se[0], se[1][:, None]))
        y = y + (pn * f32(self.const_noise)).clamp(-clip, clip)[:, None, :]
        # b. rotation
        if self.rot_deg > 0:
            axis = draws.index(H("AXIS", env, se), 3)
            unit = draws.unit(H("ANGLE", env, se)).to(dt)                                   # 2u - 1: exact
            ang = (unit * f32(self.rot_deg)) * (f32(math.pi / 180) if dt == torch.float32 else math.pi / 180)
            cs, sn = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
            a0, a1, a2 = y[..., 0], y[..., 1], y[..., 2]
            ax = axis[:, None]
            r0 = torch.where(ax == 0, a0, torch.where(ax == 1, a0 * cs - a2 * sn, a0 * cs + a1 * sn))
            r1 = torch.where(ax == 0, a1 * cs + a2 * sn, torch.where(ax == 1, a1, a1 * cs - a0 * sn))
            r2 = torch.where(ax == 0, a2 * cs - a1 * sn, torch.where(ax == 1, a0 * sn + a2 * cs, a2))
            y = torch.stack([r0, r1, r2], -1)
        # c. outliers, d. dropout: object by object
        drop_all = torch.zeros(N, Pt, dtype=torch.bool, device=dev)
        parts, off = [], 0
        for o, P in enumerate(pts):
            sl = y[:, off:off + P]
            K = int(P * self.outlier_ratio)
            if K > 0:
                lo, hi = sl.min(dim=1, keepdim=True).values, sl.max(dim=1, keepdim=True).values
                gk, ek = g[:, off:off + K], e[:, off:off + K]
                contour = H("CONTOUR", gk) < thr(self.contour_prob)
                idx = draws.index(H("INDEX", gk), P)
                free = Z("FREE", ek) * f32(self.outlier_scale)
                beyond = Z("CONTOUR", ek).abs()
                side = H("SIDE", ek) < thr(0.5)
                new = torch.where(contour[:, :, None], torch.where(side, hi + beyond, lo - beyond), free)
                w = torch.full((N, P), -1, device=dev)                                       # the highest k wins
                w.scatter_reduce_(1, idx, torch.arange(K, device=dev).expand(N, K), "amax")
                picked = torch.gather(new, 1, w.clamp(min=0)[:, :, None].expand(N, P, 3))
                sl = torch.where((w >= 0)[:, :, None], picked, sl)
            if self.dropout_ratio > 0:
                live = H("EXEMPT", env * 4 + o) < thr(1.0 - self.no_dropout_prob)
                drop_all[:, off:off + P] = (H("DROP", g[:, off:off + P]) < thr(self.dropout_ratio)) & live[:, None]
            parts.append(sl)
            off += P
        y = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
        if self.dropout_ratio > 0:
            y = torch.where(drop_all[:, :, None], torch.zeros_like(y), y)
        return torch.where(hit[:, None, None], y, x).reshape(clouds.shape)

    def fused(self, clouds, episode):
        """draw + the op; clouds above 4096 points per object take the same draws through ``apply``."""
        from .. import ops                   # registers torch.ops.mi355ppo (and loads the native library) on first use
        self.seed_step = self.draw()
        if max(self.points) > ops.PCL_AUG_MAX_POINTS:
            return self.apply(clouds, episode, self.seed_step)
        return torch.ops.mi355ppo.pcl_augment(clouds, self.points, episode, self.params(), self.seed_episode, self.seed_step)
