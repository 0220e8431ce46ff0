"""Camera depth + segmentation augmentation, host side: the reference's names (algo/models/transformer/utils.py:12-128,
280-322, 422-454), the float64 restatement the GPU tests compare against (tests/img_augment_ref.py) on hand-built cases,
``SyncTransform.draw`` / ``apply``, the default-off rule of ``Runner`` / ``ResidentLoader``, and the op's schema, fake
kernel and refusals (they raise before any launch).  No GPU."""
import math
import types

import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import img_augment_ref as R

NAMES = ("define_img_transforms", "ImageTransform", "SyncTransform", "SyncEvalTransform", "SyncCenterReshapeTransform",
         "SyncRandomCrop", "SyncCenterCrop")


def _U():
    from isaacgyminsertion_amd.algo.models.transformer import utils
    return utils


def _pair(B=3, T=2, H=19, W=27, seed=0):
    g = torch.Generator().manual_seed(seed)
    seg = torch.randint(0, 4, (B, T, 1, H, W), generator=g).float()
    return torch.rand(B, T, 1, H, W, generator=g) * (seg > 1), seg


def test_api_surface():
    U = _U()
    for n in NAMES:
        assert hasattr(U, n), n
    import algo.models.transformer.utils as shim
    for n in NAMES:
        assert getattr(shim, n) is getattr(U, n)
    five = U.define_img_transforms(60, 104, 54, 96, 16, 0.01, 0.3, rotation_deg=1.0)
    assert len(five) == 5
    transform, mask_transform, eval_transform, sync, sync_eval = five
    assert isinstance(sync, U.SyncTransform) and isinstance(sync_eval, U.SyncEvalTransform)
    assert isinstance(sync.sync_crop, U.SyncRandomCrop)
    assert (sync.rotation_deg, sync.noise_std, sync.masking_prob, sync.patch) == (1.0, 0.01, 0.3, 16)
    assert sync.size == (60, 104) and sync.crop_size == (54, 96) and not sync.is_identity
    # the reference's signature: the rotation argument is ours, and last
    assert U.define_img_transforms(54, 96, 54, 96)[3].is_identity


# ---- the restatement against hand-built cases ---------------------------------------------------------------------
def test_restatement_angle_zero_and_crop_are_slicing():
    img, seg = _pair(B=4, T=2, H=19, W=27)
    rows = torch.tensor([2, 0, 3, 2])
    h, w = 11, 13
    off = torch.tensor([[3, 5], [0, 0], [8, 14], [1, 2]], dtype=torch.int32)
    a, b, band = R.augment(img, seg, rows, off, torch.zeros(4, 2), None, h, w, 1)
    assert not band.any()
    for i in range(4):
        t, l = off[i].tolist()
        assert torch.equal(a[i], img[rows[i], ..., t:t + h, l:l + w].double())
        assert torch.equal(b[i], seg[rows[i], ..., t:t + h, l:l + w].double())
    assert torch.equal(a[0], img[2][..., 3:3 + h, 5:5 + w].double())


def test_restatement_keep_zeroes_whole_patches_of_the_image_only():
    H, W, p = 17, 23, 4
    img, seg = torch.ones(2, 1, 1, H, W), torch.ones(2, 1, 1, H, W)
    keep = torch.ones(2, H // p, W // p, dtype=torch.uint8)
    keep[0, 1, 2] = 0
    keep[1, 3, 4] = 0
    off = torch.zeros(2, 2, dtype=torch.int32)
    a, b, _ = R.augment(img, seg, torch.arange(2), off, torch.zeros(2, 2), keep, H, W, p)
    assert torch.equal(b, torch.ones_like(b))
    want = torch.ones(2, 1, 1, H, W, dtype=torch.float64)
    want[0, 0, 0, 4:8, 8:12] = 0
    want[1, 0, 0, 12:16, 16:20] = 0
    assert torch.equal(a, want)
    # remainder rows / columns (16 and 20..22) are untouched even when every patch is dropped
    a, _, _ = R.augment(img, seg, torch.arange(2), off, torch.zeros(2, 2), torch.zeros_like(keep), H, W, p)
    assert (a[..., :16, :20] == 0).all() and (a[..., 16:, :] == 1).all() and (a[..., :, 20:] == 1).all()


def test_restatement_quarter_turn_and_zero_fill():
    """A rotation by 90 degrees of a square is an exact permutation (a positive angle turns the picture counter-clockwise,
    the sense of utils._TrainAugment's theta); the rim of a small rotation reads outside the window: zeros."""
    x = torch.arange(25.).reshape(1, 1, 5, 5)
    assert torch.equal(R.rotate(x, torch.tensor([math.pi / 2])), torch.rot90(x, 1, (2, 3)).double())
    y = R.rotate(torch.ones(1, 1, 54, 96), torch.tensor([math.radians(3.0)]))
    assert y[0, 0, 0, 0] == 0 and y[0, 0, -1, -1] == 0 and y[0, 0, 27, 48] == 1
    assert 0.9 < y.mean() < 1.0


def test_near_tie_share_of_every_gpu_case():
    """The exclusion band cannot hide a failure: at most 0.5 % of the pixels of any (size, angle) case."""
    deg = sorted({a for pair in R.ROT_ANGLES_DEG for a in pair} | {0.05})
    ang = (torch.tensor(deg, dtype=torch.float64) * (math.pi / 180)).float()
    for H, W in R.ROT_SIZES + [(50, 90)]:
        share = R.tie_band(ang, H, W).double().mean(dim=(1, 2))
        print(f"{H} x {W}:", {d: f"{100 * s:.3f} %" for d, s in zip(deg, share.tolist())})
        assert (share <= R.TIE_SHARE_MAX).all(), (H, W, share)
        assert share[deg.index(0.0)] == 0


# ---- draw ---------------------------------------------------------------------------------------------------------
def test_draw_ranges_shapes_and_determinism():
    U = _U()
    sync = U.define_img_transforms(60, 104, 54, 96, 16, 0.01, 0.3, rotation_deg=1.0)[3]
    B, T = 512, 3
    off, ang, keep, seed = sync.draw(B, T, torch.Generator().manual_seed(5))
    assert off.shape == (B, 2) and off.dtype == torch.int32          # one window per sample, shared by its T frames
    assert off[:, 0].min() == 0 and off[:, 0].max() == 6 and off[:, 1].min() == 0 and off[:, 1].max() == 8
    lim = math.radians(1.0)
    assert ang.shape == (B, 2) and ang.dtype == torch.float32 and ang.abs().max() <= lim and ang.abs().max() > 0.9 * lim
    rho = torch.corrcoef(ang.T)[0, 1].abs()
    assert rho < 5 / math.sqrt(B) and not torch.equal(ang[:, 0], ang[:, 1])     # image and mask angles are independent
    assert keep.shape == (B * T, 3, 6) and keep.dtype == torch.uint8             # per frame
    assert abs(keep.float().mean() - 0.7) < 5 * math.sqrt(0.21 / keep.numel())
    assert not torch.equal(keep[0::T], keep[1::T])
    assert 0 <= seed < 2 ** 63
    again = sync.draw(B, T, torch.Generator().manual_seed(5))
    assert torch.equal(off, again[0]) and torch.equal(ang, again[1]) and torch.equal(keep, again[2]) and seed == again[3]
    other = sync.draw(B, T, torch.Generator().manual_seed(6))
    assert not torch.equal(off, other[0]) and seed != other[3]


def test_a_stage_that_is_off_draws_nothing():
    U = _U()
    g = torch.Generator().manual_seed(1)
    before = g.get_state()
    off, ang, keep, seed = U.define_img_transforms(54, 96, 54, 96)[3].draw(8, 2, g)
    assert torch.equal(g.get_state(), before)
    assert not off.any() and not ang.any() and keep is None and seed == 0
    off, ang, keep, seed = U.define_img_transforms(60, 104, 54, 96)[4].draw(8, 2, g)      # eval: the centre window
    assert torch.equal(g.get_state(), before) and off.tolist() == [[3, 4]] * 8 and not ang.any() and keep is None

    def stream_after(**kw):
        g = torch.Generator().manual_seed(1)
        U.define_img_transforms(60, 104, 54, 96, **kw)[3].draw(8, 2, g)
        return torch.rand(4, generator=g)
    crop_only = stream_after()
    # each stage that is on moves the stream; one that is off leaves it where the others put it
    assert not torch.equal(crop_only, stream_after(rotation_deg=1.0))
    assert not torch.equal(crop_only, stream_after(img_masking_prob=0.3))
    assert not torch.equal(crop_only, stream_after(img_gaussian_noise=0.01))
    assert torch.equal(crop_only, stream_after(rotation_deg=0.0, img_masking_prob=0.0, img_gaussian_noise=0.0))


# ---- default-off ---------------------------------------------------------------------------------------------------
def _runner_stub(**offline):
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config, merge
    cfg = merge(default_config(num_envs=8, horizon_length=4, rl_device="cpu"), {"offline_train": offline})
    r = Runner.__new__(Runner)
    r.task_cfg, r.cfg = cfg, cfg.offline_train
    r._init_transforms()
    return r


def test_default_config_builds_no_camera_transform():
    state = torch.random.get_rng_state()
    r = _runner_stub()
    assert r.sync_transform is None and r.sync_eval_transform is None
    assert torch.equal(torch.random.get_rng_state(), state)
    for k, v in (("img_patch_size", 16), ("img_gaussian_noise", 0.0), ("img_masking_prob", 0.0), ("img_rotation_deg", 0.0)):
        assert r.cfg.get(k) == v
    r = _runner_stub(img_width=60, img_height=104, img_crop_w=6, img_crop_h=8)
    assert r.sync_transform is not None and r.sync_eval_transform is not None
    assert (r.crop_img_width, r.crop_img_height) == (54, 96)
    r = _runner_stub(img_rotation_deg=1.0)
    assert r.sync_transform.rotation_deg == 1.0 and r.sync_eval_transform is None      # nothing cropped: eval is identity


class _Items:
    """stands in for a TactileDataset: eight fields per item, the camera pair in 1 and 2"""

    def __init__(self, n, T=2, H=6, W=8):
        g = torch.Generator().manual_seed(3)
        self.items = [(torch.zeros(1), torch.rand(T, 1, H, W, generator=g), torch.rand(T, 1, H, W, generator=g),
                       torch.rand(T, 5, generator=g), torch.rand(T, 6, generator=g), torch.rand(T, 7, generator=g),
                       torch.rand(T, 8, generator=g), torch.rand(T, 6, generator=g)) for _ in range(n)]
        self.tactile_transform = self.sync_transform = None

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_loader_without_a_transform_is_index_select():
    from isaacgyminsertion_amd.algo.models.transformer.data import ResidentLoader
    ds = _Items(11)
    dl = ResidentLoader(ds, 4, shuffle=True, device="cpu", generator=torch.Generator().manual_seed(2))
    assert dl.sync_transform is None
    order = torch.randperm(11, generator=torch.Generator().manual_seed(2))
    batches = list(dl)
    assert len(batches) == len(dl) == 3
    for k, batch in enumerate(batches):
        idx = order[4 * k:4 * k + 4]
        assert batch[0].shape == (idx.numel(), 1) and not batch[0].any()
        for j in range(1, 8):
            assert torch.equal(batch[j], torch.stack([it[j] for it in ds.items]).index_select(0, idx)), (k, j)


# ---- the torch-op classes ------------------------------------------------------------------------------------------
def test_sync_transform_apply_equals_the_restatement():
    U = _U()
    sync = U.define_img_transforms(19, 27, 17, 23, 4, 0.0, 0.3, rotation_deg=3.0)[3]
    img, seg = _pair(B=5, T=2, H=19, W=27, seed=1)
    off = torch.tensor([[0, 0], [2, 4], [1, 3], [2, 0], [0, 4]], dtype=torch.int32)
    ang = R.rot_angles()
    keep = (torch.rand(10, 4, 5, generator=torch.Generator().manual_seed(4)) >= 0.3).to(torch.uint8)
    a, b = sync.apply(img, seg, off, ang, keep)
    ra, rb, band = R.augment(img, seg, torch.arange(5), off, ang, keep, 17, 23, 4)
    assert a.shape == (5, 2, 1, 17, 23) and a.dtype == torch.float32
    assert band.double().mean() <= R.TIE_SHARE_MAX
    assert torch.equal(torch.where(band[0], ra, a.double()), ra) and torch.equal(torch.where(band[1], rb, b.double()), rb)
    assert not torch.equal(ra[3], R.sample_window(img, torch.arange(5), off, 17, 23)[3]) # it did rotate


def test_sync_transform_forward_on_an_item_and_a_batch():
    U = _U()
    sync = U.define_img_transforms(60, 104, 54, 96, 16, 0.01, 0.3, rotation_deg=1.0)[3]
    img, seg = _pair(B=2, T=3, H=60, W=104)
    torch.manual_seed(0)
    a, b = sync(img[0], seg[0])                                   # the dataset's call: (T, C, H, W)
    assert a.shape == b.shape == (3, 1, 54, 96)
    torch.manual_seed(0)
    a2, b2 = sync(img[0], seg[0])
    assert torch.equal(a, a2) and torch.equal(b, b2)
    a, b = sync(img, seg)
    assert a.shape == b.shape == (2, 3, 1, 54, 96)
    # masked patches are exactly zero in the image; the mask keeps its noise there
    zero_patches = (a.reshape(6, 54, 96)[:, :48].reshape(6, 3, 16, 6, 16).abs().amax(dim=(2, 4)) == 0)
    assert zero_patches.any() and not zero_patches.all()
    stages = U.ImageTransform(sync.img_transform)(img[..., :54, :96])
    assert stages.shape == (2, 3, 1, 54, 96)


def test_eval_transforms_are_deterministic():
    U = _U()
    _, _, eval_t, _, sync_eval = U.define_img_transforms(60, 104, 54, 96, 16, 0.01, 0.3, rotation_deg=1.0)
    img, seg = _pair(B=2, T=2, H=60, W=104)
    state = torch.random.get_rng_state()
    a, b = sync_eval(img, seg)
    assert torch.equal(torch.random.get_rng_state(), state)
    assert torch.equal(a, img[..., 3:57, 4:100]) and torch.equal(b, seg[..., 3:57, 4:100])
    a1, b1 = sync_eval(img[0], seg[0])
    assert torch.equal(a1, a[0]) and torch.equal(b1, b[0])
    assert torch.equal(eval_t(img[0]), a[0])
    c, d = U.SyncCenterCrop((54, 96))(img, seg)
    assert torch.equal(c, a) and torch.equal(d, b)
    r, s = U.SyncCenterReshapeTransform((54, 96), None, None)(a, b)           # frames already at the cropped size
    assert torch.equal(r, a) and torch.equal(s, b)
    r, s = U.SyncCenterReshapeTransform((54, 96), None, None)(img, seg)
    assert torch.equal(r, a) and torch.equal(s, b)
    crop = U.SyncRandomCrop((54, 96))
    p, q = crop(img, seg)
    i, j, h, w = crop.crop_params
    assert torch.equal(p, img[..., i:i + h, j:j + w]) and torch.equal(q, seg[..., i:i + h, j:j + w])
    assert crop(seg, img)[0].shape == p.shape and crop.crop_params == (i, j, h, w)        # kept until reset()
    crop.reset()
    assert crop.crop_params is None


# ---- the op --------------------------------------------------------------------------------------------------------
def _op_args(B=3, N=4, T=2, Hs=19, Ws=27, gh=4, gw=5):
    return dict(img=torch.zeros(N, T, 1, Hs, Ws), seg=torch.zeros(N, T, 1, Hs, Ws), rows=torch.zeros(B, dtype=torch.int64),
                offsets=torch.zeros(B, 2, dtype=torch.int32), angles=torch.zeros(B, 2),
                keep=torch.ones(B * T, gh, gw, dtype=torch.uint8), out_h=17, out_w=23, patch=4, noise_std=0.0, seed=0)


def test_op_schema_and_fake_kernel():
    from isaacgyminsertion_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "image_pair_augment" in ops.OP_NAMES
    s = str(torch.ops.mi355ppo.image_pair_augment.default._schema)
    assert s.startswith("mi355ppo::image_pair_augment(Tensor img, Tensor seg, Tensor rows, Tensor offsets, Tensor angles, "
                        "Tensor? keep, int out_h, int out_w, int patch, float noise_std, int seed)"), s
    assert s.endswith("-> (Tensor, Tensor)")
    with FakeTensorMode():
        a, b = torch.ops.mi355ppo.image_pair_augment(*_op_args().values())
        assert a.shape == b.shape == (3, 2, 1, 17, 23) and a.dtype == torch.float32
        a, _ = torch.ops.mi355ppo.image_pair_augment(*{**_op_args(), "keep": None}.values())
        assert a.shape == (3, 2, 1, 17, 23)


@pytest.mark.parametrize("change, message", [
    (dict(img=torch.zeros(4, 2, 1, 19, 27, dtype=torch.float64)), "img: expected dtype"),
    (dict(rows=torch.zeros(3, dtype=torch.int32)), "rows: expected dtype"),
    (dict(offsets=torch.zeros(3, 2, dtype=torch.int64)), "offsets: expected dtype"),
    (dict(angles=torch.zeros(3, 2, dtype=torch.float64)), "angles: expected dtype"),
    (dict(keep=torch.ones(6, 4, 5, dtype=torch.bool)), "keep: expected dtype"),
    (dict(img=torch.zeros(4, 2, 19, 27), seg=torch.zeros(4, 2, 19, 27)), "img: expected 5 dimensions"),
    (dict(rows=torch.zeros(3, 1, dtype=torch.int64)), "rows: expected 1 dimensions"),
    (dict(seg=torch.zeros(4, 2, 1, 27, 19).transpose(3, 4)), "seg: expected a contiguous"),
    (dict(offsets=torch.zeros(2, 3, dtype=torch.int32).T), "offsets: expected a contiguous"),
    (dict(seg=torch.zeros(4, 2, 1, 19, 28)), "seg: expected img's shape"),
    (dict(img=torch.zeros(4, 2, 2, 19, 27), seg=torch.zeros(4, 2, 2, 19, 27)), r"img: expected \(N, T, 1, Hs, Ws\)"),
    (dict(offsets=torch.zeros(4, 2, dtype=torch.int32)), "offsets: expected shape"),
    (dict(angles=torch.zeros(3, 1)), "angles: expected shape"),
    (dict(out_h=20), "out_h: expected 1..19"),
    (dict(out_w=28), "out_w: expected 1..27"),
    (dict(patch=0), "patch: expected >= 1"),
    (dict(keep=torch.ones(6, 4, 6, dtype=torch.uint8)), "keep: expected shape"),
    (dict(keep=torch.ones(3, 4, 5, dtype=torch.uint8)), "keep: expected shape"),
    (dict(noise_std=-0.01), "noise_std: expected >= 0"),
    (dict(noise_std=float("nan")), "noise_std: expected >= 0"),
    (dict(), "expected a HIP"),                                   # everything else right, host tensors: no CPU path
])
def test_op_refuses_bad_arguments(change, message):
    args = {**_op_args(), **change}
    with pytest.raises(RuntimeError, match=message):
        torch.ops.mi355ppo.image_pair_augment(*args.values())
