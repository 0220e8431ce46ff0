"""Point-cloud augmentation golden vectors from the REFERENCE class (build container only):
isaacgyminsertion/tasks/factory_tactile/factory_utils.py:83-166 ``PointCloudAugmentations``, loaded by file path under a
private module name.

  deterministic pieces, as written there:
    rot/*     ``random_rotate``: 5 clouds x 7 points, axes 0 / 1 / 2, angles including 0 and +-30 degrees
    offset/*  ``random_noise`` with sigma = 0: the clamped per-env offset, |pn| > 1 included so that the clamp bites
  random stages: the reference's own ``random_noise`` / ``batch_random_dropout`` / ``add_outliers`` with ``torch.rand``,
  ``torch.randn``, ``torch.randn_like`` and ``torch.randint`` replaced, for the call, by queues that hold THIS feature's hash
  draws (tests/pcl_augment_ref.py: sites, planes, element numbers) -- the golden is the reference's arithmetic on our draws.
  ``add_outliers`` draws one randn for the max side and one for the min side of every coordinate and discards one; both
  get the same tensor.  Probabilities are handed over rounded to float32, so ``u < p`` on u = hash 2^-32 is the integer
  comparison ``hash < threshold(p)`` exactly.  B = 4, P = 37 and 40, one object per cloud, every env hit, episode 0
  (the per-episode offset of the noise case is the feature's own draw too).

    python tests/golden/make_golden_pcl_augment.py  ->  tests/golden/pcl_augment.npz
"""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_harness as rh  # noqa: E402

rh.install()
from tests import pcl_augment_ref as R  # noqa: E402
from oracle.token_dropout import tok_hash  # noqa: E402

SEED_EPISODE = 4242424242424242
SEED_STEP = {"noise": 1234567890123, "dropout": 987654321987, "outliers": 5550003}


def load_reference():
    path = os.path.join(rh.REFERENCE_ROOT, "isaacgyminsertion", "tasks", "factory_tactile", "factory_utils.py")
    spec = importlib.util.spec_from_file_location("_igi_reference_factory_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PointCloudAugmentations


class Queues:
    """torch.rand / randn / randn_like / randint for the duration of a ``with``: each call pops the next prepared tensor
    of its kind and checks its shape."""

    def __init__(self, rand=(), randn=(), randint=()):
        self.q = {"rand": list(rand), "randn": list(randn), "randint": list(randint)}

    def _pop(self, kind, shape):
        t = self.q[kind].pop(0)
        assert tuple(t.shape) == tuple(shape), (kind, tuple(t.shape), tuple(shape))
        return t.clone()

    def __enter__(self):
        self.saved = (torch.rand, torch.randn, torch.randn_like, torch.randint)
        shape_of = lambda a: tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list, torch.Size)) else tuple(a)  # noqa: E731
        torch.rand = lambda *a, **k: self._pop("rand", shape_of(a))
        torch.randn = lambda *a, **k: self._pop("randn", shape_of(a))
        torch.randn_like = lambda x, **k: self._pop("randn", x.shape)
        torch.randint = lambda lo, hi, size, **k: self._pop("randint", size)
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randn, torch.randn_like, torch.randint = self.saved
        if exc[0] is None:
            assert not any(self.q.values()), {k: len(v) for k, v in self.q.items()}     # every draw was taken


def uniform(seed, site, idx):
    """u = hash 2^-32 (exact in float64): u < p for a float32 p is hash < threshold(p)."""
    return torch.from_numpy(tok_hash(seed, site, idx).astype(np.float64) * 2.0 ** -32)


if __name__ == "__main__":
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    PCA = load_reference()
    out = {}
    gen = torch.Generator().manual_seed(0)

    # ---- deterministic: random_rotate
    x = torch.randn(5, 7, 3, generator=gen, dtype=torch.float32).double() * 0.25
    angles_deg = torch.tensor([0.0, 30.0, -30.0, 12.5, -3.0])
    axes = torch.tensor([0, 1, 2, 0, 2])
    aug = PCA()
    y = aug.random_rotate(x.clone(), angles_deg * (math.pi / 180), axes)
    out["rot/x"], out["rot/angles_deg"], out["rot/axes"], out["rot/y"] = x.numpy(), angles_deg.numpy(), axes.numpy(), y.numpy()

    # ---- deterministic: the clamped per-env offset (sigma = 0)
    x = torch.randn(4, 37, 3, generator=gen, dtype=torch.float32).double() * 0.25
    pn = torch.tensor([[0.2, -0.7, 0.99], [1.5, -2.5, 0.0], [-1.0001, 1.0, 3.0], [0.5, -0.5, -1.2]])
    aug = PCA(sigma=0.0)
    with Queues(rand=[torch.zeros(4, 37)], randn=[torch.zeros(4, 37, 3)]):
        y = aug.random_noise(x.clone(), pn.unsqueeze(1))
    out["offset/x"], out["offset/pn"], out["offset/y"] = x.numpy(), pn.numpy(), y.numpy()

    # ---- random_noise on our draws: B = 4, P = 37
    B, P = 4, 37
    g = np.arange(B * P).reshape(B, P)
    e = np.arange(B * P * 3).reshape(B, P, 3)
    x = torch.randn(B, P, 3, generator=gen, dtype=torch.float32).double() * 0.25      # fp32 values: the op reads them exactly
    pn = R.gauss(R.episode_seed(SEED_EPISODE, 0), R.PLANE_PN, (B, 3))            # every env in its episode 0
    s = SEED_STEP["noise"]
    noise_prob = R.f32(0.3)
    aug = PCA()                                                  # sigma, clip, const_noise = 0.001
    with Queues(rand=[uniform(s, R.SITE_MASK, g)], randn=[R.gauss(s, R.PLANE_JITTER, (B, P, 3))]):
        y = aug.random_noise(x.clone(), pn.unsqueeze(1), noise_prob=noise_prob)
    out["noise/x"], out["noise/pn"], out["noise/y"], out["noise/seed"] = x.numpy(), pn.numpy(), y.numpy(), np.array(s)
    out["noise/seed_episode"] = np.array(SEED_EPISODE)

    # ---- batch_random_dropout on our draws: B = 4, P = 40
    B, P = 4, 40
    g = np.arange(B * P).reshape(B, P)
    x = torch.randn(B, P, 3, generator=gen, dtype=torch.float32).double() * 0.25      # fp32 values: the op reads them exactly
    s = SEED_STEP["dropout"]
    ratio, ndp = R.f32(0.2), 0.5                                 # 1 - 0.5 is a float32
    with Queues(rand=[uniform(s, R.SITE_EXEMPT, np.arange(B) * 4), uniform(s, R.SITE_DROP, g)]):
        y = aug.batch_random_dropout(x.clone(), dropout_ratio=ratio, no_dropout_prob=ndp)
    out["dropout/x"], out["dropout/y"], out["dropout/seed"] = x.numpy(), y.numpy(), np.array(s)
    out["dropout/ratio"], out["dropout/no_dropout_prob"] = np.array(ratio), np.array(ndp)
    assert 0 < int((y == 0).all(-1).sum()) < B * P

    # ---- add_outliers on our draws: B = 4, P = 40, K = 4
    ratio_o, contour_prob, scale = 0.1, 0.75, 1.5
    K = int(P * ratio_o)
    x = torch.randn(B, P, 3, generator=gen, dtype=torch.float32).double() * 0.25      # fp32 values: the op reads them exactly
    s = SEED_STEP["outliers"]
    gk, ek = g[:, :K], (g[:, :K, None] * 3 + np.arange(3))
    index = torch.from_numpy(((tok_hash(s, R.SITE_INDEX, gk) >> np.uint32(8)).astype(np.int64) * P) >> 24)
    for b in range(B):                                           # the winner rule on duplicates is ours, not scatter_'s
        assert len(set(index[b].tolist())) == K, f"seed {s}: duplicate replaced indices in cloud {b}: {index[b].tolist()}"
    side = uniform(s, R.SITE_SIDE, ek)
    beyond = R.gauss(s, R.PLANE_CONTOUR, (B * P, 3)).reshape(B, P, 3)[:, :K]
    free = R.gauss(s, R.PLANE_FREE, (B * P, 3)).reshape(B, P, 3)[:, :K]
    rand, randn = [uniform(s, R.SITE_CONTOUR, gk)], [free]
    for c in (2, 0, 1):                                          # the reference's order of coordinates
        rand.append(side[:, :, c])
        randn += [beyond[:, :, c], beyond[:, :, c]]              # max side, min side: the same tensor
    with Queues(rand=rand, randn=randn, randint=[index]):
        y = aug.add_outliers(x.clone(), outlier_ratio=ratio_o, contour_prob=contour_prob, scale_factor=scale)
    out["outliers/x"], out["outliers/y"], out["outliers/seed"] = x.numpy(), y.numpy(), np.array(s)
    out["outliers/index"] = index.numpy()

    path = os.path.join(HERE, "pcl_augment.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} KB")
