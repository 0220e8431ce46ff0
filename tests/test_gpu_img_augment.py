"""k_image_pair_augment (csrc/augment.h) through torch.ops.mi355ppo.image_pair_augment, SyncTransform.fused, the
resident loader and the Runner, against the float64 restatement tests/img_augment_ref.py.

Gather, crop and patch masking are copies and multiplications by 0 / 1: exact.  The rotation is exact on every pixel
whose float64 source coordinate is farther than 1e-4 from a rounding tie (the excluded share is asserted, <= 0.5 %).
Noise: with d = output - noise-free output of the same call,
    |d - noise_std * z_ref| <= 2e-5 * noise_std + 2^-22 * (|pixel| + 6 * noise_std)
(z is at most ~5.8 from 24-bit uniforms through precise fp32 log / sqrt / cos, a few ulp each; the second term is the
rounding of the fp32 sum and of the difference)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import img_augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _op(img, seg, rows, off, ang, keep, h, w, patch=1, noise_std=0.0, seed=0):
    d = lambda t: None if t is None else t.to(DEV)
    a, b = torch.ops.mi355ppo.image_pair_augment(d(img), d(seg), d(rows), d(off), d(ang), d(keep), h, w, patch, noise_std,
                                                 seed)
    return a.cpu(), b.cpu()


def _arenas(N, T, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    seg = torch.randint(0, 4, (N, T, 1, H, W), generator=g).float()
    return torch.rand(N, T, 1, H, W, generator=g) + 0.25, seg          # no zero in the image: zero fill is visible


ROWS = torch.tensor([3, 0, 6, 3, 5])                                      # one repeated sample
OFFSETS = {(60, 104): [[0, 0], [6, 8], [3, 4], [1, 7], [5, 2]], (19, 27): [[0, 0], [2, 4], [1, 3], [2, 0], [0, 4]]}


def test_gather_and_crop_without_rotation():
    img, seg = _arenas(7, 2, 60, 104)
    off = torch.tensor(OFFSETS[(60, 104)], dtype=torch.int32)
    a, b = _op(img, seg, ROWS, off, torch.zeros(5, 2), None, 54, 96)
    assert a.shape == b.shape == (5, 2, 1, 54, 96)
    for i in range(5):
        t, l = off[i].tolist()
        assert torch.equal(a[i], img.index_select(0, ROWS)[i, ..., t:t + 54, l:l + 96]), i
        assert torch.equal(b[i], seg.index_select(0, ROWS)[i, ..., t:t + 54, l:l + 96]), i
    # nothing cropped: a pure gather
    img, seg = _arenas(7, 2, 54, 96, seed=1)
    a, b = _op(img, seg, ROWS, torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5, 2), None, 54, 96)
    assert torch.equal(a, img.index_select(0, ROWS)) and torch.equal(b, seg.index_select(0, ROWS))


@pytest.mark.parametrize("arena, out, T", [((60, 104), (54, 96), 2), ((19, 27), (17, 23), 1)])
def test_rotation_matches_the_restatement_off_the_tie_band(arena, out, T):
    assert out in R.ROT_SIZES
    img, seg = _arenas(7, T, *arena, seed=2)
    off = torch.tensor(OFFSETS[arena], dtype=torch.int32)
    ang = R.rot_angles()
    a, b = _op(img, seg, ROWS, off, ang, None, *out)
    ra, rb, band = R.augment(img, seg, ROWS, off, ang, None, *out, 1)
    share = band.double().mean(dim=(2, 3, 4, 5))                          # per (tensor, sample)
    print("excluded share per (tensor, sample):", share.tolist())
    assert (share <= R.TIE_SHARE_MAX).all()
    assert torch.equal(torch.where(band[0], ra, a.double()), ra)
    assert torch.equal(torch.where(band[1], rb, b.double()), rb)
    win_a, win_b = R.sample_window(img, ROWS, off, *out), R.sample_window(seg, ROWS, off, *out)
    assert torch.equal(a[0].double(), win_a[0]) and torch.equal(b[0].double(), win_b[0])      # angle 0: the window
    assert torch.equal(a[2].double(), win_a[2])                                               # sample 2: mask only
    if out == (54, 96):               # (at 17 x 23 one degree moves no pixel by half a pixel: the rotation is a copy)
        assert not torch.equal(b[2].double(), win_b[2]) and not torch.equal(a[1].double(), win_a[1])
    # zero fill at the rim (3 degrees; the image has no zero of its own), even where the uncropped frame has data
    assert (a[4, :, 0, 0, 0] == 0).all() and (a[4, :, 0, -1, -1] == 0).all() and (a[4] != 0).float().mean() > 0.9
    # image and mask of one sample turn by their own angles: the restatement with the columns swapped is another picture
    sa, sb, _ = R.augment(img, seg, ROWS, off, ang.flip(1), None, *out, 1)
    assert not torch.equal(a[3].double(), sa[3]) and not torch.equal(b[3].double(), sb[3])


@pytest.mark.parametrize("arena, out, patch, T", [((60, 104), (54, 96), 16, 2), ((19, 27), (17, 23), 4, 1)])
def test_patch_masking_is_exact_and_image_only(arena, out, patch, T):
    img, seg = _arenas(7, T, *arena, seed=3)
    off = torch.tensor(OFFSETS[arena], dtype=torch.int32)
    gh, gw = out[0] // patch, out[1] // patch
    keep = (torch.rand(5 * T, gh, gw, generator=torch.Generator().manual_seed(4)) >= 0.3).to(torch.uint8)
    assert 0 < keep.sum() < keep.numel() and (T == 1 or not torch.equal(keep[0], keep[1]))   # a mask of its own per frame
    ang = torch.zeros(5, 2)
    a, b = _op(img, seg, ROWS, off, ang, keep, *out, patch)
    ra, rb, _ = R.augment(img, seg, ROWS, off, ang, keep, *out, patch)
    assert torch.equal(a.double(), ra) and torch.equal(b.double(), rb)
    assert torch.equal(b.double(), R.sample_window(seg, ROWS, off, *out))
    dropped = R.patch_mask(keep, *out, patch).reshape(5, T, 1, *out) == 0
    assert ((a == 0) == dropped).all()
    assert not dropped[..., gh * patch:, :].any() and not dropped[..., :, gw * patch:].any()  # remainder rows / columns
    # with a rotation the mask applies to the OUTPUT patches
    a, _ = _op(img, seg, ROWS, off, R.rot_angles(), keep, *out, patch)
    assert (a[dropped] == 0).all()


def test_noise_is_the_hashed_gaussian():
    out, std, seed = (54, 96), 0.01, 0x1234567890ABCDEF & (2 ** 63 - 1)
    img, seg = _arenas(7, 2, 60, 104, seed=5)
    off = torch.tensor(OFFSETS[(60, 104)], dtype=torch.int32)
    ang = R.rot_angles()
    keep = torch.ones(10, 3, 6, dtype=torch.uint8)
    keep[3, 1, 2] = 0
    clean = _op(img, seg, ROWS, off, ang, keep, *out, 16)
    noisy = _op(img, seg, ROWS, off, ang, keep, *out, 16, std, seed)
    zs = []
    for k in range(2):
        z_ref = R.gauss(seed, k, clean[k].shape)
        if k == 0:
            z_ref = z_ref * R.patch_mask(keep, *out, 16).reshape(z_ref.shape)      # noise first, then the mask
        d = noisy[k].double() - clean[k].double()
        s = float(np.float32(std))
        err = (d - s * z_ref).abs()
        bound = 2e-5 * s + 2.0 ** -22 * (clean[k].double().abs() + 6 * s)
        print(f"plane {k}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, max |z| {z_ref.abs().max():.3f}")
        assert (err <= bound).all()
        zs.append(d / s)
    assert (noisy[0][1, 1, 0, 16:32, 32:48] == 0).all()                            # frame 3 = sample 1, t = 1
    assert not torch.allclose(zs[0], zs[1], atol=1e-3)                              # image and mask noise differ
    z = zs[1].flatten()
    n = z.numel()
    print(f"mask plane: n {n}, mean z {z.mean():.5f}, var z {z.var():.5f}")
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    again = _op(img, seg, ROWS, off, ang, keep, *out, 16, std, seed)
    assert torch.equal(again[0], noisy[0]) and torch.equal(again[1], noisy[1])      # a pure function of its arguments
    other = _op(img, seg, ROWS, off, ang, keep, *out, 16, std, seed + 1)
    assert not torch.allclose(other[1], noisy[1], atol=1e-4)


def test_ragged_rows_and_offsets_read_zeros():
    N = 7
    img, seg = _arenas(N, 2, 19, 27, seed=6)
    rows = torch.tensor([2, N, 4, -1, 2])
    off = torch.tensor([[0, 0], [1, 1], [2, 4], [0, 0], [1, 2]], dtype=torch.int32)
    a, b = _op(img, seg, rows, off, torch.zeros(5, 2), None, 17, 23)
    ra, rb, _ = R.augment(img, seg, rows, off, torch.zeros(5, 2), None, 17, 23, 1)
    assert torch.equal(a.double(), ra) and torch.equal(b.double(), rb)
    assert not a[1].any() and not a[3].any() and not b[1].any() and not b[3].any()
    assert torch.equal(a[0], img[2, ..., :17, :23]) and torch.equal(a[2], img[4, ..., 2:19, 4:27])
    # windows that leave the frame: zeros there, the overlap intact; with and without a rotation
    off = torch.tensor([[-3, -5], [10, 20], [2, 4], [-40, 0], [2 ** 31 - 1, -2 ** 31]], dtype=torch.int32)
    rows = torch.tensor([2, 1, 4, 0, 2])
    for ang in (torch.zeros(5, 2), R.rot_angles()):
        a, b = _op(img, seg, rows, off, ang, None, 17, 23)
        ra, rb, band = R.augment(img, seg, rows, off, ang, None, 17, 23, 1)
        assert torch.equal(torch.where(band[0], ra, a.double()), ra) and torch.equal(torch.where(band[1], rb, b.double()), rb)
    assert not a[3].any() and not a[4].any() and a[1].any() and a[2].all()


def test_opcheck():
    img, seg = (t.to(DEV) for t in _arenas(7, 2, 19, 27, seed=7))
    keep = torch.ones(10, 4, 5, dtype=torch.uint8, device=DEV)
    args = (img, seg, ROWS.to(DEV), torch.tensor(OFFSETS[(19, 27)], dtype=torch.int32, device=DEV), R.rot_angles().to(DEV))
    tests = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
    torch.library.opcheck(torch.ops.mi355ppo.image_pair_augment, args + (keep, 17, 23, 4, 0.01, 11), test_utils=tests)
    torch.library.opcheck(torch.ops.mi355ppo.image_pair_augment, args + (None, 17, 23, 1, 0.0, 0), test_utils=tests)


# ---- the loader and the Runner ---------------------------------------------------------------------------------------
def _write_dataset(root, n_traj=2, T=36, seed=0, size=(60, 104)):
    """the _write_dataset(camera=True) pattern of tests/test_gpu_offline.py, frames of ``size``"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    for i in range(n_traj):
        end = int(rng.integers(30, T - 1))
        d = {"eef_pos": np.concatenate([rng.normal(size=(T, 3)) * 0.1,
                                        Rotation.from_rotvec(rng.normal(size=(T, 3)) * 0.3).as_matrix().reshape(T, 9)], 1),
             "socket_pos": rng.normal(size=(T, 12)) * 0.05, "noisy_socket_pos": rng.normal(size=(T, 12)) * 0.05,
             "latent": rng.normal(size=(T, 8)), "obs_hist": rng.normal(size=(T, 15)),
             "hand_joints": rng.normal(size=(T, 6)),
             "plug_hand_quat": Rotation.from_rotvec(rng.normal(size=(T, 3)) * 0.3).as_quat(),
             "plug_hand_pos": rng.normal(size=(T, 3)) * 0.01, "plug_pos_error": rng.normal(size=(T, 3)),
             "plug_quat_error": rng.normal(size=(T, 4))}
        d["action"] = np.tanh(np.concatenate([d["eef_pos"][:, :3] * 8, d["socket_pos"][:, :3] * 10], 1))
        d = {k: v.astype(np.float32) for k, v in d.items()}
        done = np.zeros(T, dtype=bool)
        done[end] = True
        d["done"] = done
        folder = os.path.join(root, "w0", f"traj{i}", "obs")
        os.makedirs(folder)
        np.savez(os.path.join(folder, "obs.npz"), **d)
        for name in ("img", "seg"):
            os.makedirs(os.path.join(root, "w0", f"traj{i}", name))
        for t in range(T):
            # blocky segmentation (8 x 8 cells) so that a mask pixel and its neighbours mostly agree
            ids = np.kron(rng.integers(0, 4, size=(1, (size[0] + 7) // 8, (size[1] + 7) // 8)),
                          np.ones((1, 8, 8)))[:, :size[0], :size[1]].astype(np.float32)
            np.savez(os.path.join(root, "w0", f"traj{i}", "img", f"img_{t}.npz"),
                     img=(rng.random(size=(1,) + size) + 0.25).astype(np.float32))
            np.savez(os.path.join(root, "w0", f"traj{i}", "seg", f"seg_{t}.npz"), seg=ids)


def _runner(**offline):
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config, merge
    cfg = default_config(num_envs=8, horizon_length=4, rl_device=DEV)
    over = {"model": {"linear": {"input_size": 18}, "use_img": True, "use_seg": True},
            "train": dict(epochs=1, train_test_split=0.5, learning_rate=1e-3, train_batch_size=16, val_batch_size=16)}
    over.update(offline)
    return Runner(merge(cfg, {"offline_train": over}), agent=None)


def _dataset(data, seq=1):
    from isaacgyminsertion_amd.algo.models.transformer.data import DataNormalizer, TactileDataset
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device=DEV)
    files = sorted(glob.glob(os.path.join(data, "*/*/obs/*.npz")))
    norm = DataNormalizer(cfg.offline_train, files, data)
    norm.run()
    return TactileDataset(norm.file_list, sequence_length=seq, stats=norm.stats, include_img=True, include_seg=True,
                          include_tactile=False, obs_keys=cfg.offline_train.train.obs_keys)


def test_resident_loader_with_a_sync_transform(tmp_path):
    from isaacgyminsertion_amd.algo.models.transformer.data import ResidentLoader
    from isaacgyminsertion_amd.algo.models.transformer.utils import define_img_transforms
    _write_dataset(str(tmp_path), n_traj=1, T=36, seed=3)
    ds = _dataset(str(tmp_path), seq=2)

    def loader(seed, **kw):
        sync = define_img_transforms(60, 104, 54, 96, 16, **kw)[3]
        return ResidentLoader(ds, 8, shuffle=True, device=DEV, generator=torch.Generator().manual_seed(seed),
                              sync_transform=sync)

    # crop + masking (no rotation, no noise): an image pixel can only be non-zero where the logged mask is
    dl = loader(1, img_masking_prob=0.3)
    plain = ResidentLoader(ds, 8, shuffle=True, device=DEV, generator=torch.Generator().manual_seed(1))
    assert plain.fields[1].shape[-2:] == (60, 104) and torch.equal(dl.fields[1], plain.fields[1])     # stored as logged
    for batch in dl:
        img, seg = batch[1], batch[2]
        assert img.shape == seg.shape == (img.shape[0], 2, 1, 54, 96)
        assert (img[seg == 0] == 0).all() and (img != 0).any()
        assert set(seg.unique().tolist()) <= {0.0, 2.0, 3.0}
    # everything on, a seeded generator: two loaders give the same batches, another seed does not
    full = dict(img_gaussian_noise=0.01, img_masking_prob=0.3, rotation_deg=1.0)
    one, two, other = list(loader(7, **full)), list(loader(7, **full)), list(loader(8, **full))
    assert len(one) == len(two) == len(dl) and len(one) >= 2
    for x, y in zip(one, two):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert not torch.equal(one[0][1], other[0][1])
    # one launch per batch builds both tensors; the five other resident fields are still index_select
    from torch.profiler import ProfilerActivity, profile
    dl = loader(7, **full)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        n_batches = len(list(dl))
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    resident = sum(f is not None for f in dl.fields)
    assert resident == 7
    assert sum(n == "mi355ppo::image_pair_augment" for n in names) == n_batches
    assert sum(n == "aten::index_select" for n in names) == (resident - 2) * n_batches
    assert sum("k_image_pair_augment" in n for n in names) == n_batches


def test_runner_trains_and_predicts_on_cropped_augmented_frames(tmp_path):
    data = tmp_path / "data"
    _write_dataset(str(data), n_traj=2, T=36, seed=2)
    r = _runner(img_width=60, img_height=104, img_crop_w=6, img_crop_h=8, img_rotation_deg=1.0, img_gaussian_noise=0.01,
                img_masking_prob=0.3)
    assert r.sync_transform is not None and r.sync_eval_transform is not None
    r.cfg.data_folder, r.cfg.output_dir = str(data), str(tmp_path / "out")
    r.run()
    assert len(r.train_loss) == 1 and np.isfinite(r.train_loss[0]) and np.isfinite(r.val_loss[0])
    obs = {"img": torch.rand(3, 1, 54 * 96), "seg": torch.rand(3, 1, 54 * 96), "student_obs": torch.randn(3, 1, 18)}
    out, _ = r.predict(obs)
    assert out.shape == (3, 6) and torch.isfinite(out).all()
    bad = _runner(img_width=60, img_height=104, img_crop_w=4, img_crop_h=8)
    with pytest.raises(NotImplementedError, match="cropped camera images"):
        bad.predict({"img": torch.rand(3, 1, 56 * 96), "seg": torch.rand(3, 1, 56 * 96), "student_obs": torch.randn(3, 1, 18)})


def test_default_config_batches_are_todays(tmp_path):
    from isaacgyminsertion_amd.algo.models.transformer.data import ResidentLoader
    data = tmp_path / "data"
    _write_dataset(str(data), n_traj=1, T=36, seed=4, size=(54, 96))
    r = _runner()
    assert r.sync_transform is None and r.sync_eval_transform is None
    ds = _dataset(str(data))
    r.stats = ds.stats
    files = sorted(glob.glob(str(data / "*/*/obs/*.npz")))
    dl = r._make_loader(files, 16, True)
    assert dl.sync_transform is None
    torch.manual_seed(3)
    first = next(iter(dl))
    torch.manual_seed(3)
    want = next(iter(ResidentLoader(ds, 16, shuffle=True, device=DEV)))
    assert all(torch.equal(p, q) for p, q in zip(first, want))
