"""Tactile augmentation of the offline student, host side: the float64 restatement the GPU tests compare against
(tests/tactile_augment_ref.py) on hand-built cases, ``TactileAugment.draw`` / ``apply``, the blur that the fused path leaves
out, the ``offline_train.tactile_augment`` key of ``Runner`` with its default-off rule, and the op's schema, fake kernel and
refusals (they raise before any launch).  No GPU."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import tactile_augment_ref as R

NAMES = ("TactileAugment", "define_tactile_augment", "define_tactile_transforms", "TactileTransform", "GaussianNoise",
         "Masking")


def _U():
    from isaacgyminsertion_amd.algo.models.transformer import utils
    return utils


def _arena(N=4, T=2, Fg=3, H=9, W=13, seed=0, dtype=torch.float32):
    return (torch.rand(N, T, Fg, 1, H, W, generator=torch.Generator().manual_seed(seed), dtype=dtype) * 2 - 1)


def _no_jitter(n):
    j = torch.ones(n, 3)
    j[:, 0] = 0
    return j


def test_api_surface():
    U = _U()
    import algo.models.transformer.utils as shim
    for n in NAMES:
        assert hasattr(U, n), n
        assert getattr(shim, n) is getattr(U, n)
    train, ev = U.define_tactile_augment(32, 64, 28, 56, 8, 0.001, 0.3)
    assert isinstance(train, U.TactileAugment) and isinstance(ev, U.TactileAugment)
    assert train.training and not ev.training
    assert train.size == ev.size == (32, 64) and train.crop_size == ev.crop_size == (28, 56)
    assert (train.patch, train.noise_std, train.masking_prob) == (8, 0.001, 0.3)
    assert (ev.noise_std, ev.masking_prob) == (0.0, 0.0)
    assert not train.is_identity and not ev.is_identity
    train, ev = U.define_tactile_augment(32, 64, 32, 64)
    assert not train.is_identity and ev.is_identity          # the train transform always jitters and rotates
    assert hasattr(train, "fused") and not hasattr(U.define_tactile_transforms(32, 64, 32, 64)[0], "fused")
    with pytest.raises(ValueError, match="larger than the image"):
        U.TactileAugment((32, 64), (33, 64))


# ---- the restatement against hand-built cases ---------------------------------------------------------------------
def test_restatement_windows_at_the_edge_and_beyond():
    arena = _arena()
    rows = torch.tensor([2, 0])
    n = 2 * 6
    off = torch.zeros(n, 2, dtype=torch.int32)
    off[0] = torch.tensor([4, 7])             # flush with the bottom-right corner: rows 4..8, columns 7..12
    off[1] = torch.tensor([6, 10])            # two rows and three columns past it
    off[2] = torch.tensor([-2, -3])           # before the top-left corner
    off[3] = torch.tensor([9, 0])             # wholly below the frame
    off[7] = torch.tensor([1, 2])             # second sample, plane 1: a window of its own
    y = R.window(arena, rows, off, 5, 6)
    assert y.shape == (n, 1, 5, 6) and y.dtype == torch.float64
    planes = arena.reshape(4, 6, 9, 13).double()
    assert torch.equal(y[0, 0], planes[2, 0, 4:9, 7:13])
    assert torch.equal(y[1, 0, :3, :3], planes[2, 1, 6:9, 10:13]) and not y[1, 0, 3:].any() and not y[1, 0, :, 3:].any()
    assert torch.equal(y[2, 0, 2:, 3:], planes[2, 2, 0:3, 0:3]) and not y[2, 0, :2].any() and not y[2, 0, :, :3].any()
    assert not y[3].any()
    assert torch.equal(y[7, 0], planes[0, 1, 1:6, 2:8]) and torch.equal(y[6, 0], planes[0, 0, 0:5, 0:6])
    # a sample number outside the arena reads zeros
    y = R.window(arena, torch.tensor([4, -1]), off, 5, 6)
    assert not y.any()


def test_restatement_jitter_clamps_at_both_ends():
    x = torch.tensor([[-0.5, 0.0, 0.25, 0.5], [0.75, 0.95, 1.0, -1.0]]).reshape(1, 2, 4)      # frame differences: negatives
    y = R.jitter_image(x, 1.1, 1.1)
    z = torch.tensor([0.0, 0.0, 0.275, 0.55, 0.825, 1.0, 1.0, 0.0], dtype=torch.float64)       # 0.95 * 1.1 > 1; negatives -> 0
    m = z.mean()
    want = ((z - m) * 1.1 + m).clamp(0, 1)
    assert torch.allclose(y.reshape(-1), want, rtol=0, atol=1e-15)
    assert y.reshape(-1)[0] == 0 and y.reshape(-1)[5] == 1          # (0 - m) c + m < 0 and (1 - m) c + m > 1: clamped again
    assert 0 < y.reshape(-1)[2] < 0.275                              # below the mean: pushed away from it
    # flag off: the image passes as it is, negatives and all
    imgs = torch.stack([x, x]).double()
    out = R.jitter_images(imgs, torch.tensor([[0.0, 1.1, 1.1], [1.0, 1.1, 1.1]]))
    f = torch.tensor(1.1)                                            # the factors arrive as fp32 and are widened exactly
    assert torch.equal(out[0], imgs[0]) and torch.equal(out[1], R.jitter_image(x, f, f))
    assert float(f) != 1.1 and (out[1] - y).abs().max() < 1e-7
    # c < 1 pulls towards the mean; b = c = 1 is the clamp alone
    assert torch.equal(R.jitter_image(x, 1.0, 1.0), x.double().clamp(0, 1))


def test_restatement_small_rotation_reads_zeros_at_the_rim():
    y = R.rotate(torch.ones(1, 1, 32, 64, dtype=torch.float64), torch.tensor([math.radians(3.0)]))
    assert y[0, 0, 0, 0] == 0 and y[0, 0, -1, -1] == 0 and y[0, 0, 16, 32] == 1 and 0.9 < y.mean() < 1.0
    arena = torch.ones(1, 1, 1, 1, 32, 64)
    one = torch.zeros(1, 2, dtype=torch.int32)
    out, band = R.augment(arena, torch.tensor([0]), one, _no_jitter(1), torch.tensor([math.radians(3.0)]), None, 32, 64, 1)
    assert torch.equal(out.reshape(32, 64), y[0, 0]) and band.double().mean() <= R.TIE_SHARE_MAX
    # angle 0 is a copy, with no band
    out, band = R.augment(arena, torch.tensor([0]), one, _no_jitter(1), torch.zeros(1), None, 32, 64, 1)
    assert torch.equal(out, arena.double()) and not band.any()


def test_restatement_order_is_jitter_then_rotation():
    arena = _arena(N=1, T=1, Fg=1, H=32, W=64, seed=1)
    jit = torch.tensor([[1.0, 1.1, 0.9]])
    ang = torch.tensor([math.radians(3.0)])
    off = torch.zeros(1, 2, dtype=torch.int32)
    out, _ = R.augment(arena, torch.tensor([0]), off, jit, ang, None, 32, 64, 1)
    w = R.window(arena, torch.tensor([0]), off, 32, 64)
    assert torch.equal(out.reshape(1, 1, 32, 64), R.rotate(R.jitter_images(w, jit), ang))
    # the other order fills the rim with zeros first, which moves the mean
    assert not torch.equal(out.reshape(1, 1, 32, 64), R.jitter_images(R.rotate(w, ang), jit))


def test_restatement_keep_with_a_partial_last_patch():
    H, W, p = 9, 13, 4
    arena = torch.ones(1, 1, 2, 1, H, W)
    keep = torch.ones(2, H // p, W // p, dtype=torch.uint8)
    keep[0, 1, 2] = 0
    keep[1, 0, 0] = 0
    out, _ = R.augment(arena, torch.tensor([0]), torch.zeros(2, 2, dtype=torch.int32), _no_jitter(2), torch.zeros(2), keep,
                       H, W, p)
    want = torch.ones(2, H, W, dtype=torch.float64)
    want[0, 4:8, 8:12] = 0
    want[1, 0:4, 0:4] = 0
    assert torch.equal(out.reshape(2, H, W), want)
    out, _ = R.augment(arena, torch.tensor([0]), torch.zeros(2, 2, dtype=torch.int32), _no_jitter(2), torch.zeros(2),
                       torch.zeros_like(keep), H, W, p)
    out = out.reshape(2, H, W)
    assert (out[:, :8, :12] == 0).all() and (out[:, 8:, :] == 1).all() and (out[:, :, 12:] == 1).all()


def test_jitter_bound_is_what_the_issue_expects():
    assert R.jitter_bound(2048) < 5e-7 and R.jitter_bound(8192) < 1e-6
    assert R.jitter_bound(117) < R.jitter_bound(1568) < R.jitter_bound(2048)


# ---- apply ----------------------------------------------------------------------------------------------------------
ANGLES_DEG = [0, 3, -3, 1.7, -0.37, 2.5, -1, 0.05]


def _draws(n, h, w, ch, cw, patch, seed=0, masking=True):
    g = torch.Generator().manual_seed(seed)
    off = torch.stack([torch.randint(0, h - ch + 1, (n,), generator=g), torch.randint(0, w - cw + 1, (n,), generator=g)],
                      1).to(torch.int32)
    jit = torch.ones(n, 3)
    jit[:, 0] = (torch.arange(n) % 2 == 0).float()
    jit[:, 1:] = torch.where(jit[:, :1] != 0, 0.9 + 0.2 * torch.rand(n, 2, generator=g), jit[:, 1:])
    ang = (torch.tensor([ANGLES_DEG[i % 8] for i in range(n)], dtype=torch.float64) * (math.pi / 180)).float()
    keep = (torch.rand(n, ch // patch, cw // patch, generator=g) >= 0.3).to(torch.uint8) if masking else None
    return off, jit, ang, keep


@pytest.mark.parametrize("size, crop, patch", [((32, 64), (28, 56), 8), ((9, 13), (9, 13), 4), ((12, 17), (9, 13), 4)])
def test_apply_in_float64_equals_the_restatement(size, crop, patch):
    U = _U()
    aug = U.TactileAugment(size, crop, patch, 0.0, 0.3)
    x = _arena(N=3, T=2, Fg=3, H=size[0], W=size[1], seed=2, dtype=torch.float64)
    n = 18
    off, jit, ang, keep = _draws(n, *size, *crop, patch)
    rows = torch.arange(3)
    # without the jitter: slicing, a permutation with zero fill and a 0 / 1 product -- equal, off the tie band
    y = aug.apply(x, off, _no_jitter(n), ang, keep)
    ref, band = R.augment(x, rows, off, _no_jitter(n), ang, keep, *crop, patch)
    assert y.shape == (3, 2, 3, 1, *crop) and y.dtype == torch.float64
    assert band.double().mean() <= R.TIE_SHARE_MAX
    assert torch.equal(torch.where(band, ref, y), ref)
    # with it: the two float64 means may be summed in another order, 2^-52 apart per addition -- nothing else differs
    y = aug.apply(x, off, jit, ang, keep)
    ref, band = R.augment(x, rows, off, jit, ang, keep, *crop, patch)
    err = torch.where(band, torch.zeros_like(ref), (y - ref).abs())
    assert err.max() <= 1e-13
    flat_y, flat_x = y.reshape(n, *crop), R.window(x, rows, off, *crop).reshape(n, *crop)
    for i in range(1, n, 2):                                   # jitter flag off
        if ang[i] == 0:
            m = R.patch_mask(keep, *crop, patch)[i, 0]
            assert torch.equal(flat_y[i], flat_x[i] * m)


def test_apply_in_float32_and_its_noise():
    U = _U()
    size, crop, patch = (32, 64), (28, 56), 8
    aug = U.TactileAugment(size, crop, patch, 0.05, 0.3)
    x = _arena(N=3, T=1, Fg=3, H=32, W=64, seed=3)
    n = 9
    off, jit, ang, keep = _draws(n, *size, *crop, patch, seed=1)
    seed = 0x1234567890ABCDEF & (2 ** 63 - 1)
    clean = aug.apply(x, off, jit, ang, keep)
    ref, band = R.augment(x, torch.arange(3), off, jit, ang, keep, *crop, patch)
    assert clean.dtype == torch.float32
    err = torch.where(band, torch.zeros_like(ref), (clean.double() - ref).abs())
    assert err.max() <= 1e-6                                    # fp32 arithmetic of the jitter; everything else is exact
    # the noise is the kernel's hash: float64 apply against the float64 Box-Muller of the restatement
    x64 = x.double()
    noisy = aug.apply(x64, off, jit, ang, keep, 0.05, seed)
    base = aug.apply(x64, off, jit, ang, keep)
    z = R.gauss(seed, R.NOISE_PLANE, (n, 1, *crop)) * R.patch_mask(keep, *crop, patch)
    assert ((noisy - base).reshape(n, 1, *crop) - 0.05000000074505806 * z).abs().max() <= 1e-12
    assert torch.equal(aug.apply(x64, off, jit, ang, keep, 0.05, seed), noisy)
    assert not torch.allclose(aug.apply(x64, off, jit, ang, keep, 0.05, seed + 1), noisy, atol=1e-4)
    # and it is not the camera pair's field
    assert not torch.allclose(R.gauss(seed, 0, (n, 1, *crop)), R.gauss(seed, R.NOISE_PLANE, (n, 1, *crop)), atol=1e-3)


def test_forward_draws_from_the_global_cpu_generator():
    U = _U()
    train, ev = U.define_tactile_augment(32, 64, 28, 56, 8, 0.01, 0.3)
    x = _arena(N=2, T=2, Fg=3, H=32, W=64, seed=4)
    torch.manual_seed(0)
    a = train(x.reshape(-1, 1, 32, 64))                        # the loader's and TactileTransform's call: (n, C, H, W)
    torch.manual_seed(0)
    b = train(x)
    assert a.shape == (12, 1, 28, 56) and b.shape == (2, 2, 3, 1, 28, 56) and torch.equal(a.reshape(b.shape), b)
    assert not torch.equal(train(x), b)
    state = torch.random.get_rng_state()
    c = ev(x)
    assert torch.equal(torch.random.get_rng_state(), state) and torch.equal(c, x[..., 2:30, 4:60])
    assert torch.equal(U.TactileTransform(ev)(x), c)


# ---- draw -----------------------------------------------------------------------------------------------------------
def test_draw_ranges_independence_and_determinism():
    U = _U()
    aug = U.TactileAugment((32, 64), (28, 56), 8, 0.001, 0.3)
    n = 4000
    off, jit, ang, keep, seed = aug.draw(n, torch.Generator().manual_seed(5))
    assert off.shape == (n, 2) and off.dtype == torch.int32
    assert off[:, 0].min() == 0 and off[:, 0].max() == 4 and off[:, 1].min() == 0 and off[:, 1].max() == 8
    assert len({tuple(o) for o in off.tolist()}) == 5 * 9          # every image its own window: all 45 occur in 4000
    assert jit.shape == (n, 3) and jit.dtype == torch.float32 and set(jit[:, 0].tolist()) == {0.0, 1.0}
    on = jit[:, 0] != 0
    assert (jit[~on, 1:] == 1).all()
    assert jit[on, 1:].min() >= 0.9 and jit[on, 1:].max() <= 1.1 and jit[on, 1:].min() < 0.91 and jit[on, 1:].max() > 1.09
    assert not torch.equal(jit[on, 1], jit[on, 2])
    assert ang.shape == (n,) and ang.dtype == torch.float32
    turned = ang != 0
    lim = math.radians(3.0)
    assert ang.abs().max() <= lim and ang.abs().max() > 0.99 * lim and ang.min() < 0 < ang.max()
    for flags, p in ((on, 0.3), (turned, 0.5)):                   # within 5 binomial standard deviations
        assert abs(int(flags.sum()) - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (int(flags.sum()), p)
    both = int((on & turned).sum())                               # the two flags are independent draws
    assert abs(both - n * 0.15) <= 5 * math.sqrt(n * 0.15 * 0.85)
    assert keep.shape == (n, 3, 7) and keep.dtype == torch.uint8
    assert abs(keep.float().mean() - 0.7) < 5 * math.sqrt(0.21 / keep.numel()) and not torch.equal(keep[0], keep[1])
    assert isinstance(seed, int) and 0 <= seed < 2 ** 63
    again = aug.draw(n, torch.Generator().manual_seed(5))
    assert all(torch.equal(p, q) for p, q in zip((off, jit, ang, keep), again[:4])) and seed == again[4]
    other = aug.draw(n, torch.Generator().manual_seed(6))
    assert not torch.equal(off, other[0]) and not torch.equal(jit, other[1]) and seed != other[4]
    # the op's record: top, left, flag, and the bits of b, c, angle
    words = aug.pack(off, jit, ang)
    assert words.shape == (n, ops.TACTILE_AUG_WORDS) and words.dtype == torch.int32
    assert torch.equal(words[:, :2], off) and torch.equal(words[:, 2], on.to(torch.int32))
    assert torch.equal(words[:, 3:5].contiguous().view(torch.float32), jit[:, 1:])
    assert torch.equal(words[:, 5].contiguous().view(torch.float32), ang)


def test_a_stage_that_is_off_draws_nothing():
    U = _U()

    def stream_after(crop=(32, 64), noise=0.0, masking=0.0):
        g = torch.Generator().manual_seed(1)
        U.TactileAugment((32, 64), crop, 8, noise, masking).draw(8, g)
        return torch.rand(4, generator=g)
    base = stream_after()
    assert not torch.equal(base, stream_after(crop=(28, 64)))
    assert not torch.equal(base, stream_after(crop=(32, 56)))
    assert not torch.equal(base, stream_after(noise=0.001))
    assert not torch.equal(base, stream_after(masking=0.3))
    # crop, noise and masking off: the generator stands where the jitter and the rotation alone leave it
    g = torch.Generator().manual_seed(1)
    torch.rand(3, 8, generator=g)
    torch.rand(2, 8, generator=g)
    assert torch.equal(base, torch.rand(4, generator=g))
    off, jit, ang, keep, seed = U.TactileAugment((32, 64), (32, 64)).draw(8, torch.Generator().manual_seed(1))
    assert not off.any() and keep is None and seed == 0
    # evaluation: the centre window, every flag off, the generator's state untouched
    g = torch.Generator().manual_seed(1)
    before = g.get_state()
    off, jit, ang, keep, seed = U.TactileAugment((32, 64), (28, 56), 8, 0.001, 0.3, train=False).draw(8, g)
    assert torch.equal(g.get_state(), before)
    assert off.tolist() == [[2, 4]] * 8 and not jit[:, 0].any() and (jit[:, 1:] == 1).all() and not ang.any()
    assert keep is None and seed == 0


# ---- the blur the fused path leaves out --------------------------------------------------------------------------------
def _blur(x, sigma):
    """the blur stage of utils._TrainAugment.forward, flag on for every image, sigma fixed"""
    n, dev = x.shape[0], x.device
    sigma = torch.full((n,), sigma, device=dev, dtype=x.dtype)
    t = torch.arange(-2, 3, device=dev, dtype=x.dtype)
    k1 = torch.exp(-0.5 * (t[None, :] / sigma[:, None]) ** 2)
    k1 = k1 / k1.sum(1, keepdim=True)
    C = x.shape[1]
    xp = F.pad(x, (2, 2, 2, 2), mode='reflect').reshape(1, n * C, x.shape[2] + 4, x.shape[3] + 4)
    kh = k1.repeat_interleave(C, 0)
    xp = F.conv2d(xp, kh[:, None, :, None], groups=n * C)
    xp = F.conv2d(xp, kh[:, None, None, :], groups=n * C)
    return xp.reshape(n, C, *x.shape[2:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_omitted_blur_moves_no_pixel(dtype):
    x = torch.rand(12, 1, 32, 64, generator=torch.Generator().manual_seed(7), dtype=dtype) * 2 - 1
    moved = (_blur(x, 0.1) - x).abs().max()                       # sigma 0.1 is the widest kernel _TrainAugment draws
    print(f"{dtype}: the blur at sigma 0.1 moves a pixel by at most {moved:.3e}")
    assert moved <= 1e-21
    assert torch.equal(_blur(x, 0.01), x)


# ---- Runner: the key, default off ---------------------------------------------------------------------------------------
def _runner_stub(**offline):
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config, merge
    cfg = merge(default_config(num_envs=8, horizon_length=4, rl_device="cpu"), {"offline_train": offline})
    r = Runner.__new__(Runner)
    r.task_cfg, r.cfg = cfg, cfg.offline_train
    r._init_transforms()
    return r


class _Items:
    """stands in for a TactileDataset: eight fields per item, the tactile frames in field 0"""

    def __init__(self, n, T=1, Fg=3, C=1, H=32, W=64):
        g = torch.Generator().manual_seed(3)
        self.items = [(torch.rand(T, Fg, C, H, W, generator=g), torch.zeros(1), torch.zeros(1),
                       torch.rand(T, 5, generator=g), torch.rand(T, 6, generator=g), torch.rand(T, 7, generator=g),
                       torch.rand(T, 8, generator=g), torch.rand(T, 6, generator=g)) for _ in range(n)]
        self.tactile_transform = self.sync_transform = None

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _loader_of(r, monkeypatch, train=True, **items):
    from isaacgyminsertion_amd.algo.models.transformer import runner as runner_mod
    monkeypatch.setattr(runner_mod, "TactileDataset", lambda **kw: _Items(6, **items))
    r.device, r.sequence_length, r.stats = "cpu", 1, None
    r.cfg.model.use_tactile = True
    return r._make_loader([], 4, train)


def test_key_absent_builds_todays_objects(monkeypatch):
    U = _U()
    from isaacgyminsertion_amd.utils.config import default_config
    assert default_config(num_envs=8, horizon_length=4).offline_train.tactile_augment == "torch"
    r = _runner_stub()
    del r.cfg["tactile_augment"]                                   # a config written before the key existed
    state = torch.random.get_rng_state()
    r._init_transforms()
    assert torch.equal(torch.random.get_rng_state(), state)
    assert r.tactile_augment_mode == "torch" and r.tactile_augment is None and r.tactile_eval_augment is None
    kinds = [type(m) for m in r.tactile_transform]
    assert isinstance(r.tactile_transform, nn.Sequential)
    assert kinds == [U._Resize, U._Crop, U._TrainAugment, U.GaussianNoise]         # stock config: noise 0.001, no masking
    assert [type(m) for m in r.tactile_eval_transform] == [U._Resize, U._Crop]
    assert r.process_tactile.tactile_transform is r.tactile_transform
    dl = _loader_of(r, monkeypatch)
    assert dl.tactile_transform is r.tactile_transform and not hasattr(dl.tactile_transform, "fused")
    assert _loader_of(r, monkeypatch, train=False).tactile_transform is r.tactile_eval_transform
    # and the loader's batch is index_select + that object, from torch's global stream
    dl.generator = torch.Generator().manual_seed(2)
    torch.manual_seed(5)
    first = next(iter(dl))[0]
    idx = torch.randperm(6, generator=torch.Generator().manual_seed(2))[:4]
    torch.manual_seed(5)
    want = r.tactile_transform(dl.fields[0].index_select(0, idx).reshape(-1, 1, 32, 64)).reshape(4, 1, 3, 1, 32, 64)
    assert torch.equal(first, want)


def test_the_keys_three_outcomes(monkeypatch):
    U = _U()
    r = _runner_stub(tactile_augment="torch")
    assert r.tactile_augment is None and isinstance(r.tactile_transform, nn.Sequential)
    r = _runner_stub(tactile_augment="fused", tactile_crop_w=4, tactile_crop_h=8, tactile_masking_prob=0.3,
                     tactile_patch_size=8)
    assert isinstance(r.tactile_augment, U.TactileAugment) and isinstance(r.tactile_eval_augment, U.TactileAugment)
    assert r.tactile_augment.training and not r.tactile_eval_augment.training
    assert r.tactile_augment.size == (32, 64) and r.tactile_augment.crop_size == (28, 56)
    assert (r.tactile_augment.patch, r.tactile_augment.noise_std, r.tactile_augment.masking_prob) == (8, 0.001, 0.3)
    assert isinstance(r.tactile_transform, nn.Sequential)          # predict's and the dataset's objects are still there
    assert _loader_of(r, monkeypatch).tactile_transform is r.tactile_augment
    assert _loader_of(r, monkeypatch, train=False).tactile_transform is r.tactile_eval_augment
    for bad in ("Fused", "native", "", None, True):
        with pytest.raises(ValueError, match="offline_train.tactile_augment"):
            _runner_stub(tactile_augment=bad)


def test_fused_refuses_what_it_does_not_build(monkeypatch):
    with pytest.raises(NotImplementedError, match="offline_train.tactile_augment"):
        _runner_stub(tactile_augment="fused", tactile_type="rgb")
    r = _runner_stub(tactile_augment="fused")
    with pytest.raises(NotImplementedError, match="offline_train.tactile_augment.*does not resize"):
        _loader_of(r, monkeypatch, H=40, W=64)                     # stored at another size: a resize
    with pytest.raises(NotImplementedError, match="offline_train.tactile_augment.*single-channel"):
        _loader_of(r, monkeypatch, C=3)
    _runner_stub(tactile_augment="torch", tactile_type="rgb")     # the torch path takes both


def test_loader_calls_fused_with_its_generator():
    from isaacgyminsertion_amd.algo.models.transformer.data import ResidentLoader
    calls = []

    class Spy:
        def fused(self, arena, rows, generator):
            calls.append((arena, rows.clone(), generator))
            return arena.index_select(0, rows)[..., :5, :7]

    g = torch.Generator().manual_seed(2)
    dl = ResidentLoader(_Items(6), 4, shuffle=True, device="cpu", generator=g, tactile_transform=Spy())
    batches = list(dl)
    order = torch.randperm(6, generator=torch.Generator().manual_seed(2))
    assert len(calls) == 2 and all(c[0] is dl.fields[0] and c[2] is g for c in calls)
    assert torch.equal(calls[0][1], order[:4]) and torch.equal(calls[1][1], order[4:])
    assert batches[0][0].shape == (4, 1, 3, 1, 5, 7) and batches[1][0].shape == (2, 1, 3, 1, 5, 7)
    assert torch.equal(batches[0][3], dl.fields[3].index_select(0, order[:4]))


# ---- the op --------------------------------------------------------------------------------------------------------------
def _op_args(B=3, N=4, T=2, Fg=3, Hs=9, Ws=13, gh=2, gw=3):
    n = B * T * Fg
    return dict(arena=torch.zeros(N, T, Fg, 1, Hs, Ws), rows=torch.zeros(B, dtype=torch.int64),
                params=torch.zeros(n, 6, dtype=torch.int32), keep=torch.ones(n, gh, gw, dtype=torch.uint8), out_h=9,
                out_w=13, patch=4, noise_std=0.0, seed=0)


def test_op_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "tactile_augment" in ops.OP_NAMES
    s = str(torch.ops.mi355ppo.tactile_augment.default._schema)
    assert s == ("mi355ppo::tactile_augment(Tensor arena, Tensor rows, Tensor params, Tensor? keep, int out_h, int out_w, "
                 "int patch, float noise_std, int seed) -> Tensor"), s
    with FakeTensorMode():
        y = torch.ops.mi355ppo.tactile_augment(*_op_args().values())
        assert y.shape == (3, 2, 3, 1, 9, 13) and y.dtype == torch.float32
        y = torch.ops.mi355ppo.tactile_augment(*{**_op_args(), "keep": None, "out_h": 5, "out_w": 6}.values())
        assert y.shape == (3, 2, 3, 1, 5, 6)


def test_c_abi_python_binding_and_cpp_registration_agree():
    import os
    import re
    from isaacgyminsertion_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "igi_ppo.h")).read()
    capi = open(os.path.join(root, "isaacgyminsertion_amd", "csrc", "igi_capi.hip")).read()
    cpp = open(os.path.join(root, "isaacgyminsertion_amd", "csrc", "torch_ops.cpp")).read()
    assert "igi_tactile_augment" in _lib.exported_symbols()
    assert re.search(r"^int igi_tactile_augment\(", hdr, re.M) and re.search(r"^int igi_tactile_augment\(", capi, re.M)
    assert f"#define IGI_TACTILE_AUG_WORDS {ops.TACTILE_AUG_WORDS}" in hdr
    args = len(_lib._EXPORTS["igi_tactile_augment"][1])
    decl = re.search(r"^int igi_tactile_augment\((.*?)\);", hdr, re.M | re.S).group(1)
    assert args == len(decl.split(",")) == 16
    schema = str(torch.ops.mi355ppo.tactile_augment.default._schema).replace("mi355ppo::", "")
    assert f'm.def("{schema}");' in cpp and 'm.impl("tactile_augment", tactile_augment);' in cpp


@pytest.mark.parametrize("change, message", [
    (dict(arena=torch.zeros(4, 2, 3, 1, 9, 13, dtype=torch.float64)), "arena: expected dtype"),
    (dict(rows=torch.zeros(3, dtype=torch.int32)), "rows: expected dtype"),
    (dict(params=torch.zeros(18, 6)), "params: expected dtype"),
    (dict(keep=torch.ones(18, 2, 3, dtype=torch.bool)), "keep: expected dtype"),
    (dict(arena=torch.zeros(4, 6, 1, 9, 13)), "arena: expected 6 dimensions"),
    (dict(rows=torch.zeros(3, 1, dtype=torch.int64)), "rows: expected 1 dimensions"),
    (dict(params=torch.zeros(18 * 6, dtype=torch.int32)), "params: expected 2 dimensions"),
    (dict(arena=torch.zeros(4, 2, 3, 1, 13, 9).transpose(4, 5)), "arena: expected a contiguous"),
    (dict(params=torch.zeros(6, 18, dtype=torch.int32).T), "params: expected a contiguous"),
    (dict(keep=torch.ones(18, 3, 2, dtype=torch.uint8).transpose(1, 2)), "keep: expected a contiguous"),
    (dict(arena=torch.zeros(4, 2, 3, 3, 9, 13)), r"arena: expected \(N, T, F, 1, Hs, Ws\)"),
    (dict(arena=torch.zeros(0, 2, 3, 1, 9, 13)), r"arena: expected \(N, T, F, 1, Hs, Ws\) non-empty"),
    (dict(params=torch.zeros(17, 6, dtype=torch.int32)), "params: expected shape"),
    (dict(params=torch.zeros(18, 5, dtype=torch.int32)), "params: expected shape"),
    (dict(params=torch.zeros(3, 6, dtype=torch.int32)), "params: expected shape"),        # one row per IMAGE, not per sample
    (dict(out_h=10), "out_h: expected 1..9"),
    (dict(out_h=0), "out_h: expected 1..9"),
    (dict(out_w=14), "out_w: expected 1..13"),
    (dict(patch=0), "patch: expected >= 1"),
    (dict(keep=torch.ones(18, 2, 4, dtype=torch.uint8)), "keep: expected shape"),
    (dict(keep=torch.ones(3, 2, 3, dtype=torch.uint8)), "keep: expected shape"),
    (dict(noise_std=-0.001), "noise_std: expected >= 0"),
    (dict(noise_std=float("nan")), "noise_std: expected >= 0"),
    (dict(), "expected a HIP"),                                   # everything else right, host tensors: no CPU path
])
def test_op_refuses_bad_arguments(change, message):
    args = {**_op_args(), **change}
    with pytest.raises(RuntimeError, match=message):
        torch.ops.mi355ppo.tactile_augment(*args.values())


def test_patch_zero_without_a_keep_grid_is_not_looked_at():
    with pytest.raises(RuntimeError, match="expected a HIP"):     # past every argument check: refused for the device alone
        torch.ops.mi355ppo.tactile_augment(*{**_op_args(), "keep": None, "patch": 0}.values())
