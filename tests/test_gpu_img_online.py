"""k_image_pair_augment_seeded (csrc/augment_seeded.h) through torch.ops.mi355ppo.image_pair_augment_seeded,
SyncTransform.fused_seeded and ExtrinsicAdapt's distillation step, against the float64 restatement tests/img_online_ref.py
(layered on tests/img_augment_ref.py).

Arenas of horizon * envs = 6 flat rows; T = 1 and 2; frames 54 x 96 (two bands, 16-byte stores), 17 x 23 (scalar stores, a
partial last group; patch 4: partial patches, patch 16: a 1 x 1 grid) and 8 x 8 with a cell per pixel; batches of 5 rows with
one repeated row and one row outside the arena; one case of 67 rows; depth only, mask only, and both.  Seeds: ``O.SEEDS``,
chosen on the CPU (tests/test_img_online_cpu.py asserts the tie share of every one of them).

The draws are exact: ``draws`` is ``torch.equal`` to the restatement's.  The pixel chain is held to the bounds of
tests/test_gpu_img_augment.py, unchanged: gather and patch masking exact; the rotation exact on every pixel whose float64
source coordinate is farther than 1e-4 from a rounding tie; and with d = output - noise-free output of the same call,
|d - noise_std * z_ref| <= 2e-5 * noise_std + 2^-22 * (|pixel| + 6 * noise_std)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import img_augment_ref as A
from tests import img_online_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = torch.tensor(O.ROWS)
CASE_IDS = [f"T{T}-{H}x{W}-p{p}" for T, H, W, p, _rot in O.CASES]


def _flat(a):
    return None if a is None else a.reshape(a.shape[0], -1).contiguous().to(DEV)


def _op(img, seg, rows, patch, noise_std=0.0, masking_prob=0.0, rot=0.0, seed=0, want_draws=False):
    some = img if img is not None else seg
    T, (H, W) = some.shape[1], some.shape[-2:]
    outs = torch.ops.mi355ppo.image_pair_augment_seeded(_flat(img), _flat(seg), rows.to(DEV), T, H, W, patch, noise_std,
                                                        masking_prob, O.max_rad(rot), seed, want_draws)
    return tuple(None if o is None else o.cpu() for o in outs)


def _gathered(arena, rows=ROWS):
    """index_select with the row outside the arena read as zeros."""
    live = rows < arena.shape[0]
    out = torch.zeros(rows.numel(), *arena.shape[1:])
    out[live] = arena.index_select(0, rows[live])
    return out


def _noise_bound(base, std):
    s = float(np.float32(std))
    return 2e-5 * s + 2.0 ** -22 * (base.double().abs() + 6 * s)


@pytest.fixture(scope="module")
def clean():
    """Every case x seed with the rotation alone, computed once: (img, seg, the op's outputs, the restatement's)."""
    out = {}
    for k, (T, H, W, patch, rot) in enumerate(O.CASES):
        img, seg = O.arena(T, H, W, seed=2 * k), O.arena(T, H, W, seed=2 * k + 1)
        for seed in O.SEEDS:
            yi, ys, d = _op(img, seg, ROWS, patch, rot=rot, seed=seed, want_draws=True)
            ri, rs, band, draws = O.augment(img, seg, ROWS, seed, patch, rotation_deg=rot)
            out[(k, seed)] = (img, seg, yi, ys, d, ri, rs, band, draws)
    return out


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_draws_are_the_restatements_bit_for_bit(clean, k):
    from isaacgyminsertion_amd.algo.models.transformer.utils import define_img_transforms
    T, H, W, patch, rot = O.CASES[k]
    for seed in O.SEEDS:
        img, seg, yi, ys, d, _ri, _rs, _band, (_off, ang, _keep) = clean[(k, seed)]
        assert yi.shape == ys.shape == (5, T, 1, H, W) and d.shape == (5, 2) and d.dtype == torch.int32
        assert torch.equal(d, O.angle_bits(ang)) and (d != 0).all()
        aug = define_img_transforms(H, W, H, W, patch, 0.01, 0.3, rot)[3]
        assert torch.equal(d, aug.draw_seeded(5, T, seed)[1].view(torch.int32))              # SyncTransform.draw_seeded
        # identical whether one tensor or two are present; and each tensor's pixels do not depend on the other's presence
        y1, none, d1 = _op(img, None, ROWS, patch, rot=rot, seed=seed, want_draws=True)
        none2, y2, d2 = _op(None, seg, ROWS, patch, rot=rot, seed=seed, want_draws=True)
        assert none is None and none2 is None and torch.equal(d1, d) and torch.equal(d2, d)
        assert torch.equal(y1, yi) and torch.equal(y2, ys)
        # nor on whether they are asked for, nor on noise or masking
        y3, _s3, d3 = _op(img, seg, ROWS, patch, rot=rot, seed=seed)
        assert d3 is None and torch.equal(y3, yi)
        assert torch.equal(_op(img, seg, ROWS, patch, 0.01, 0.3, rot, seed, True)[2], d)


@pytest.mark.parametrize("present", ["both", "img", "seg"])
@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_everything_off_is_the_two_gathers(clean, k, present):
    T, H, W, patch, _rot = O.CASES[k]
    img, seg = clean[(k, O.SEEDS[0])][:2]
    yi, ys, d = _op(img if present != "seg" else None, seg if present != "img" else None, ROWS, patch, seed=O.SEEDS[0],
                    want_draws=True)
    assert not d.any()                                                # max_rad 0: no hash, the copy path
    if present != "seg":
        assert torch.equal(yi, _gathered(img)) and (yi < 0).any() and not yi[4].any()
    else:
        assert yi is None
    if present != "img":
        assert torch.equal(ys, _gathered(seg)) and not ys[4].any()
    else:
        assert ys is None


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_masked_cells_are_zero_kept_cells_untouched_and_the_mask_tensor_is_never_masked(clean, k):
    T, H, W, patch, rot = O.CASES[k]
    seed = O.SEEDS[k % len(O.SEEDS)]
    img, seg, yi, ys, _d, _ri, _rs, _band, _draws = clean[(k, seed)]
    gh, gw = H // patch, W // patch
    keep = O.draws(5, T, seed, H, W, patch, 0.3, rot)[2]
    mask = A.patch_mask(keep, H, W, patch).reshape(yi.shape)
    if gh * gw > 1:
        assert 0 < keep.sum() < keep.numel() and len({tuple(g.flatten().tolist()) for g in keep}) > 1
    # without a rotation: the gather times the mask, exactly; the mask tensor: the gather
    mi, ms, _ = _op(img, seg, ROWS, patch, 0.0, 0.3, 0.0, seed)
    assert torch.equal(mi.double(), _gathered(img).double() * mask) and torch.equal(ms, _gathered(seg))
    # after the rotation: exact zeros, and the kept cells bit for bit
    mi, ms, _ = _op(img, seg, ROWS, patch, 0.0, 0.3, rot, seed)
    assert torch.equal(mi.double(), yi.double() * mask) and torch.equal(ms, ys)
    dropped = mask == 0
    assert not dropped[..., gh * patch:, :].any() and not dropped[..., :, gw * patch:].any()   # past the last whole patch: kept
    # depth alone: the same cells
    assert torch.equal(_op(img, None, ROWS, patch, 0.0, 0.3, rot, seed)[0], mi)
    # after noise the mask still zeroes the OUTPUT cells, of the depth frames only
    ni, ns, _ = _op(img + 1.5, seg + 1.5, ROWS, patch, 0.05, 0.3, 0.0, seed)
    assert (ni[dropped] == 0).all() and (ni[:4][~dropped[:4]] != 0).float().mean() > 0.99 and (ns[:4] != 0).float().mean() > 0.99
    # masking_prob 1 keeps nothing but the rows and columns past the last whole patch
    a1, s1, _ = _op(img + 1.5, seg + 1.5, ROWS, patch, 0.0, 1.0, 0.0, seed)
    assert not a1[..., :gh * patch, :gw * patch].any() and torch.equal(s1, _gathered(seg + 1.5))
    if (H, W) == (17, 23):
        edge = gh * patch, gw * patch
        assert edge == ((16, 20) if patch == 4 else (16, 16))
        assert a1[:4][..., edge[0]:, :].all() and a1[:4][..., :, edge[1]:].all()


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_rotation_alone_equals_the_restatement_off_the_tie_band(clean, k):
    T, H, W, _patch, rot = O.CASES[k]
    moved = swapped_differs = 0
    for seed in O.SEEDS:
        img, seg, yi, ys, _d, ri, rs, band, (_off, ang, _keep) = clean[(k, seed)]
        share = float(band.double().mean())
        print(f"{CASE_IDS[k]} seed {seed}: excluded share {share:.5f}")
        assert share <= O.TIE_SHARE_MAX
        for w, (y, r, x) in enumerate(((yi, ri, img), (ys, rs, seg))):
            assert torch.equal(torch.where(band[w], r, y.double()), r)
            assert not y[4].any()                                     # the row outside the arena: zeros
            moved += int((y[:4] != _gathered(x)[:4]).flatten(1).any(1).sum())
        # depth and mask have their own angles: the restatement with the two columns exchanged is another picture
        assert not torch.equal(ang[:, 0], ang[:, 1])
        sw_i, sw_s, sw_band = A.augment(img, seg, ROWS, torch.zeros(5, 2, dtype=torch.int32), ang.flip(1), None, H, W, 1)
        swapped_differs += int(not torch.equal(torch.where(band[0] | sw_band[0], sw_i, yi.double()), sw_i))
        swapped_differs += int(not torch.equal(torch.where(band[1] | sw_band[1], sw_s, ys.double()), sw_s))
        # the T frames of a sample share the angle: frame t alone, rotated by the sample's angle
        if T == 2:
            for t in range(T):
                one = A.rotate(_gathered(img)[:, t].double(), ang[:, 0])          # (5, 1, H, W)
                assert torch.equal(torch.where(band[0][:, t], one, yi[:, t].double()), one)
    assert moved >= 4 and swapped_differs >= 2                         # the turns do move pixels at this size


@pytest.mark.parametrize("k, std", [(0, 0.01), (1, 0.05), (2, 0.01), (3, 0.05), (4, 0.05)],
                         ids=["T1-54x96-0.01", "T2-54x96-0.05", "T1-17x23-0.01", "T2-17x23-0.05", "T2-8x8-0.05"])
def test_noise_is_the_hashed_gaussian_of_planes_zero_and_one(clean, k, std):
    T, H, W, patch, rot = O.CASES[k]
    seed = O.SEEDS[1]
    img, seg, bi, bs, _d, _ri, _rs, _band, (off, ang, _keep) = clean[(k, seed)]
    ni, ns, _ = _op(img, seg, ROWS, patch, std, 0.0, rot, seed)
    s = float(np.float32(std))
    ds = []
    for plane, (noisy, base) in enumerate(((ni, bi), (ns, bs))):
        z_ref = A.gauss(seed, plane, base.shape)
        d = noisy.double() - base.double()
        err = (d - s * z_ref).abs()
        bound = _noise_bound(base, std)
        print(f"{CASE_IDS[k]} std {std} plane {plane}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
        assert (d - s * A.gauss(seed, 1 - plane, base.shape)).abs().max() > std            # not the other tensor's plane
        assert (d - s * A.gauss(seed, 2, base.shape)).abs().max() > std                    # nor the tactile plane
        # mean and variance of d / s over n pixels: within 5 standard deviations (1 / sqrt(n), sqrt(2 / n))
        n, zs = d.numel(), d / s
        assert abs(float(zs.mean())) <= 5 / math.sqrt(n) and abs(float(zs.var()) - 1) <= 5 * math.sqrt(2 / n)
        ds.append(d)
    assert (ds[0] - ds[1]).abs().max() > std                           # depth and mask noise differ
    # the row outside the arena: zeros plus noise
    assert (ni[4].double() - s * A.gauss(seed, 0, bi.shape)[4]).abs().max() <= 2e-5 * s + 2.0 ** -22 * 6 * s
    other = _op(img, seg, ROWS, patch, std, 0.0, rot, seed + 1)[0]
    assert not torch.allclose(other, ni, atol=0.1 * std)
    # one tensor alone: the same noise at the same index
    assert torch.equal(_op(None, seg, ROWS, patch, std, 0.0, rot, seed)[1], ns)
    # what k_image_pair_augment gives for the same seed, index and angles: the same bits, plane 0 and plane 1
    r5 = lambda a: a.to(DEV)                                           # noqa: E731
    oi, os_ = torch.ops.mi355ppo.image_pair_augment(r5(img), r5(seg), r5(ROWS), r5(off), r5(ang), None, H, W, patch, std, seed)
    assert torch.equal(oi.cpu(), ni) and torch.equal(os_.cpu(), ns)


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_the_whole_chain_stays_within_the_bounds(clean, k):
    T, H, W, patch, rot = O.CASES[k]
    std, p_mask = 0.05, 0.3
    for seed in O.SEEDS[:2]:
        img, seg = clean[(k, seed)][:2]
        yi, ys, d = _op(img, seg, ROWS, patch, std, p_mask, rot, seed, True)
        ri, rs, band, (_off, ang, keep) = O.augment(img, seg, ROWS, seed, patch, std, p_mask, rot)
        ci, cs, _b, _dr = O.augment(img, seg, ROWS, seed, patch, 0.0, 0.0, rot)         # the pixel the noise is added to
        assert torch.equal(d, O.angle_bits(ang))
        for w, (y, r, c) in enumerate(((yi, ri, ci), (ys, rs, cs))):
            err = torch.where(band[w], torch.zeros_like(r), (y.double() - r).abs())
            assert (err <= _noise_bound(c, std)).all()
        dropped = A.patch_mask(keep, H, W, patch).reshape(yi.shape) == 0
        assert (yi[dropped] == 0).all() and (ys[:4] != 0).float().mean() > 0.99


def test_sixty_seven_rows():
    B, T, H, W, patch, rot = O.MANY
    img, seg = O.arena(T, H, W, seed=20), O.arena(T, H, W, seed=21)
    rows = (torch.arange(B) * 5) % (O.ARENA_ROWS + 1)              # every row, the one outside the arena included
    for seed in O.SEEDS[:2]:
        yi, ys, d = _op(img, seg, rows, patch, 0.0, 0.3, rot, seed, True)
        ri, rs, band, (_off, ang, _keep) = O.augment(img, seg, rows, seed, patch, 0.0, 0.3, rot)
        assert torch.equal(d, O.angle_bits(ang)) and band.double().mean() <= O.TIE_SHARE_MAX
        assert torch.equal(torch.where(band[0], ri, yi.double()), ri) and torch.equal(torch.where(band[1], rs, ys.double()), rs)
        assert not yi[rows == O.ARENA_ROWS].any() and not ys[rows == O.ARENA_ROWS].any() and (rows == O.ARENA_ROWS).sum() >= 5


def test_repeats_are_bit_identical_and_the_inputs_are_untouched():
    T, H, W, patch, rot = O.CASES[1]
    img, seg = _flat(O.arena(T, H, W, seed=4)), _flat(O.arena(T, H, W, seed=5))
    before = img.clone(), seg.clone()
    rows = ROWS.to(DEV)
    op = torch.ops.mi355ppo.image_pair_augment_seeded
    call = lambda seed, r=rows: op(img, seg, r, T, H, W, patch, 0.01, 0.3, O.max_rad(rot), seed, True)     # noqa: E731
    a, b, c = call(O.SEEDS[0]), call(O.SEEDS[0]), call(O.SEEDS[1])
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(img, before[0]) and torch.equal(seg, before[1])
    assert all(not torch.equal(x, y) for x, y in zip(a, c))
    # rows in another order: sample b's draws go with its place in the batch, its pixels with its row
    assert torch.equal(call(O.SEEDS[0], rows.flip(0))[2], a[2])
    # the repeated row (places 0 and 3): the same frames under two angle pairs
    assert not torch.equal(a[0][0], a[0][3]) and not torch.equal(a[2][0], a[2][3])
    e = call(1, rows[:0])
    assert e[0].shape == e[1].shape == (0, T, 1, H, W) and e[2].shape == (0, 2)


def test_a_grid_above_8192_cells_is_refused_and_fused_seeded_takes_the_torch_path():
    from isaacgyminsertion_amd import _lib
    from isaacgyminsertion_amd.algo.models.transformer.utils import define_img_transforms
    g = torch.Generator().manual_seed(0)
    big_i, big_s = torch.rand(2, 9216, generator=g).to(DEV), torch.rand(2, 9216, generator=g).to(DEV)
    rows = torch.tensor([1, 0], device=DEV)
    op = torch.ops.mi355ppo.image_pair_augment_seeded
    with pytest.raises(RuntimeError, match="igi_image_pair_augment_seeded"):
        op(big_i, big_s, rows, 1, 96, 96, 1, 0.0, 0.3, 0.0, 1, False)             # 96 x 96 cells of one pixel = 9216
    op(big_i, big_s, rows, 1, 96, 96, 1, 0.0, 0.0, 0.0, 1, False)                 # without masking there is no grid
    aug = define_img_transforms(96, 96, 96, 96, 1, 0.01, 0.3, 3.0)[3]
    yi, ys, d = aug.fused_seeded(big_i, big_s, rows, O.SEEDS[0], want_draws=True)
    off, ang, keep, s = aug.draw_seeded(2, 1, O.SEEDS[0])
    assert yi.shape == ys.shape == (2, 1, 1, 96, 96) and torch.isfinite(yi).all() and d.device == yi.device
    assert torch.equal(d.cpu(), O.angle_bits(ang)) and torch.equal(d.cpu(), O.angle_bits(O.draws(2, 1, O.SEEDS[0], 96, 96, 1, 0.3, 3.0)[1]))
    wi, ws = aug.apply_seeded(big_i[rows].reshape(2, 1, 1, 96, 96), big_s[rows].reshape(2, 1, 1, 96, 96), off, ang, keep, 0.01, s)
    assert torch.equal(yi, wi) and torch.equal(ys, ws)
    # 8192 cells is the largest grid the kernel takes: 64 x 128 cells of one pixel
    edge = torch.rand(1, 1, 1, 64, 128, generator=g)
    zero = torch.zeros(1, dtype=torch.int64)
    yi, _none, _d = _op(edge, None, zero, 1, 0.0, 0.3, 0.0, O.SEEDS[0])
    keep = O.draws(1, 1, O.SEEDS[0], 64, 128, 1, 0.3, 0.0)[2]
    assert torch.equal(yi.double(), edge.double() * A.patch_mask(keep, 64, 128, 1).reshape(edge.shape)) and 0 < keep.sum() < 8192
    # fused_seeded on the kernel's path is the op on the arenas as the gather sees them
    T, H, W, patch, rot = O.CASES[1]
    img, seg = _flat(O.arena(T, H, W, seed=4)), _flat(O.arena(T, H, W, seed=5))
    aug = define_img_transforms(H, W, H, W, patch, 0.01, 0.3, rot)[3]
    got = aug.fused_seeded(img, seg, ROWS.to(DEV), O.SEEDS[2], want_draws=True)
    want = op(img, seg, ROWS.to(DEV), T, H, W, patch, 0.01, 0.3, O.max_rad(rot), O.SEEDS[2], True)
    assert got[0].shape == (5, T, 1, H, W) and all(torch.equal(x, y) for x, y in zip(got, want))
    only = aug.fused_seeded(None, seg, ROWS.to(DEV), O.SEEDS[2], want_draws=True)
    assert only[0] is None and torch.equal(only[1], want[1]) and torch.equal(only[2], want[2])
    # the C entry refuses an output that is an arena (the op allocates its outputs, so only a C caller can ask): no launch
    p = lambda t: C.c_void_p(t.data_ptr())                             # noqa: E731
    fn = _lib.lib().igi_image_pair_augment_seeded
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, rows_dev = torch.empty(5, T, 1, H, W, device=DEV), ROWS.to(DEV)
    before = img.clone()
    for oi, os_ in ((p(img), p(out)), (p(seg), p(out)), (p(out), p(img)), (p(out), p(seg)), (p(out), p(out))):
        assert fn(p(img), p(seg), 6, T, H, W, p(rows_dev), 5, patch, 0.0, 0.0, 0.0, C.c_uint64(1), oi, os_, None,
                  stream) == _lib.IGI_E_BADARG
    assert fn(None, None, 6, T, H, W, p(rows_dev), 5, patch, 0.0, 0.0, 0.0, C.c_uint64(1), None, None, None,
              stream) == _lib.IGI_E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(img, before)


def test_opcheck():
    T, H, W, patch, rot = O.CASES[3]
    img, seg = _flat(O.arena(T, H, W, seed=7)), _flat(O.arena(T, H, W, seed=8))
    tests = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
    op = torch.ops.mi355ppo.image_pair_augment_seeded
    torch.library.opcheck(op, (img, seg, ROWS.to(DEV), T, H, W, patch, 0.01, 0.3, O.max_rad(rot), 11, True), test_utils=tests)
    torch.library.opcheck(op, (None, seg, ROWS.to(DEV), T, H, W, 1, 0.0, 0.0, 0.0, 0, False), test_utils=tests)
    torch.library.opcheck(op, (img, None, ROWS.to(DEV), T, H, W, 4, 0.0, 0.3, 0.0, 3, True), test_utils=tests)


# ---- the trainer ----------------------------------------------------------------------------------------------------------
E = O.ENGINE
STEPS = E["mini_epochs"] * E["mini_epochs"]                          # optimizer steps per epoch: 4 minibatches x 4 mini-epochs
MB = E["envs"] * E["horizon"] // E["mini_epochs"]
ARENA = E["envs"] * E["horizon"]
HW = E["hw"]


def _agent(key, img_info=True, seg_info=True, tactile=False, seed=0):
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=E["envs"], horizon_length=E["horizon"], rl_device=DEV, mini_epochs=E["mini_epochs"],
                         obs_info=True, tactile_info=tactile, pcl_info=False, img_info=img_info, seg_info=seg_info,
                         num_points=8)
    assert cfg.seed == E["seed"]
    off = cfg.offline_train
    off.img_rotation_deg, off.img_gaussian_noise = E["rotation_deg"], E["noise_std"]
    off.img_masking_prob, off.img_patch_size = E["masking_prob"], E["patch"]
    if key is None:
        off.pop("img_augment_online")
    else:
        off.img_augment_online = key
    if tactile:
        off.tactile_augment_online = "fused"
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    env = SyntheticInsertionEnv(E["envs"], device=DEV, tactile_hw=(32, 64) if tactile else None, pcl_points=0, img_hw=HW)
    agent = ExtrinsicAdapt(env, None, cfg)
    agent.obs = env.reset()
    return agent, env


def _profiled(fn):
    """-> (every event's name, the device kernels' names in launch order)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = prof.events()
    return [e.name for e in ev], [e.name for e in ev if e.device_type == DeviceType.CUDA and "mem" not in e.name.lower()]


def _rollout(agent):
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    agent.set_student_eval()
    return _profiled(agent.play_steps)


@pytest.mark.parametrize("infos", [(True, True), (False, True)], ids=["img_info+seg_info", "seg_info"])
def test_trainer_with_the_key_on(monkeypatch, infos):
    from isaacgyminsertion_amd.algo.ppo import experience
    img_info, seg_info = infos
    agent, _env = _agent("fused", img_info, seg_info)
    aug = agent.img_augment
    assert aug is not None and (aug.patch, aug.noise_std, aug.masking_prob, aug.rotation_deg) == (16, 0.01, 0.3, 1.0)
    names, _kernels = _rollout(agent)
    assert not any("image_pair_augment_seeded" in n for n in names)                      # the rollout: none of it
    assert agent.img_seed is None
    store = agent.storage.storage_dict
    assert ("n_img" in store) == img_info and "n_seg" in store
    stored = {k: store[k].clone() for k in ("n_img", "n_seg") if k in store}
    calls, fused, prefetched, batches = [], aug.fused_seeded, [], []

    def spy(img2d, seg2d, rows, seed, want_draws=False):
        yi, ys, _ = fused(img2d, seg2d, rows, seed, want_draws)
        calls.append((img2d, seg2d, rows.clone(), seed, None if yi is None else yi.detach().clone(), ys.detach().clone()))
        return yi, ys, None
    aug.fused_seeded = spy
    prefetch, getitem = experience._LazyMinibatch.prefetch, experience.StudentBuffer.__getitem__

    def spy_prefetch(self, keys):
        prefetched.append(keys)
        return prefetch(self, keys)

    def spy_getitem(self, i):
        batches.append(getitem(self, i))
        return batches[-1]
    monkeypatch.setattr(experience._LazyMinibatch, "prefetch", spy_prefetch)
    monkeypatch.setattr(experience.StudentBuffer, "__getitem__", spy_getitem)
    # one optimizer step under the profiler: one launch of the kernel, and the gather no longer moves the camera rows
    agent.set_student_train()
    names, kernels = _profiled(lambda: agent.update_step(0))
    assert sum("k_image_pair_augment_seeded" in n for n in names) == 1
    assert sum(n == "mi355ppo::image_pair_augment_seeded" for n in names) == 1
    assert sum(n == "mi355ppo::gather_rows" for n in names) == 1
    assert not {"n_img", "n_seg"} & set(prefetched[0]) and "n_student_obs" in prefetched[0]
    assert not {"n_img", "n_seg"} & set(batches[0]._c) and "n_student_obs" in batches[0]._c      # never gathered
    agent.optim.step(1.0)
    # a whole epoch's update: one launch per optimizer step
    names, kernels = _profiled(agent.update)
    assert sum("k_image_pair_augment_seeded" in n for n in names) == STEPS and len(calls) == 1 + STEPS
    assert [c[3] for c in calls] == O.engine_seeds(1 + STEPS) and agent.img_seed == calls[-1][3]
    for k, v in stored.items():
        assert torch.equal(store[k], v)                                                   # the arenas are read in place
    # the step's camera input is the restatement's for the recorded seeds, within the unchanged bounds
    cpu = {k: v.reshape(ARENA, 1, 1, *HW).cpu() for k, v in stored.items()}
    for img2d, seg2d, rows, seed, yi, ys in calls[:5]:
        assert (img2d is None) == (not img_info) and seg2d.data_ptr() == store["n_seg"].data_ptr()
        assert seg2d.shape == (ARENA, HW[0] * HW[1]) and rows.numel() == MB
        if img_info:
            assert img2d.data_ptr() == store["n_img"].data_ptr() and img2d.shape == seg2d.shape
        ri, rs, band, (_off, _ang, keep) = O.augment(cpu.get("n_img"), cpu["n_seg"], rows.cpu(), seed, E["patch"],
                                                     E["noise_std"], E["masking_prob"], E["rotation_deg"])
        ci, cs, _b, _d = O.augment(cpu.get("n_img"), cpu["n_seg"], rows.cpu(), seed, E["patch"], 0.0, 0.0, E["rotation_deg"])
        assert band.double().mean() <= O.TIE_SHARE_MAX
        for w, (y, r, c) in enumerate(((yi, ri, ci), (ys, rs, cs))):
            if y is None:
                assert w == 0 and not img_info
                continue
            assert y.shape == (MB, 1, 1, *HW)
            err = torch.where(band[w], torch.zeros_like(r), (y.cpu().double() - r).abs())
            assert (err <= _noise_bound(c, E["noise_std"])).all()
        if img_info:
            dropped = A.patch_mask(keep, *HW, E["patch"]).reshape(yi.shape) == 0
            assert dropped.any() and (yi.cpu()[dropped] == 0).all()
    aug.fused_seeded = fused
    monkeypatch.undo()
    # one whole train_epoch: rollout (unaugmented) + update
    agent.obs = _env.reset()
    action_losses, _latent = agent.train_epoch()
    assert len(action_losses) == STEPS and all(bool(torch.isfinite(l).all()) for l in action_losses)


def test_one_train_epoch_with_the_tactile_key_on_too():
    agent, _env = _agent("fused", tactile=True)
    assert agent.img_augment is not None and agent.tactile_augment is not None
    assert agent.img_augment.generator is not agent.tactile_augment.generator
    agent.set_student_eval()
    names, _kernels = _profiled(agent.train_epoch)
    assert sum("k_image_pair_augment_seeded" in n for n in names) == STEPS
    assert sum("k_tactile_augment_seeded" in n for n in names) == STEPS
    assert agent.img_seed == O.engine_seeds(STEPS)[-1] == agent.tactile_seed            # equal seeds, different sites


def test_trainer_with_the_key_off_is_the_trainer_without_it():
    results = []
    for key in (None, "off"):
        agent, _env = _agent(key)
        assert agent.img_augment is None and agent.img_seed is None
        _rollout(agent)
        agent.set_student_train()
        loss, _ = agent.update_step(0)
        agent.optim.step(1.0)
        names, kernels = _profiled(lambda: agent.update_step(1))
        assert not any("image_pair_augment_seeded" in n for n in names)
        results.append((loss.detach().clone(), kernels, agent.storage.storage_dict["n_img"].clone(),
                        agent.storage.storage_dict["n_seg"].clone()))
    assert torch.equal(results[0][0], results[1][0]) and bool(torch.isfinite(results[0][0]).all())
    assert results[0][1] == results[1][1] and len(results[0][1]) > 10
    assert torch.equal(results[0][2], results[1][2]) and torch.equal(results[0][3], results[1][3])


def test_the_train_entry_runs_with_the_key(tmp_path):
    """``python -m isaacgyminsertion_amd.train train.algo=ExtrinsicAdapt ... offline_train.img_augment_online=fused``: two
    epochs of 64 envs x 8 steps on the synthetic env; without a camera modality the key is refused by name."""
    from isaacgyminsertion_amd import train as T
    small = ["task.env.numEnvs=64", "train.ppo.horizon_length=8", "train.ppo.mini_epochs=2", "task.rl.max_episode_length=16",
             "train.network.mlp.units=[64,48,32]", "train.network.priv_mlp.units=[48,32,8]", f"output_root={tmp_path}",
             "train.algo=ExtrinsicAdapt", "offline_train.img_augment_online=fused", "train.ppo.max_agent_steps=1500"]
    with pytest.raises(ValueError, match="offline_train.img_augment_online.*img_info or train.ppo.seg_info"):
        T.run(T.build_config(None, small))
    agent = T.run(T.build_config(None, small + ["train.ppo.img_info=True", "train.ppo.seg_info=True",
                                                "offline_train.img_gaussian_noise=0.01", "offline_train.img_rotation_deg=1.0",
                                                "offline_train.img_masking_prob=0.3"]))
    assert agent.img_augment is not None and agent.agent_steps >= 1500 and agent.epoch_num == 2
    assert agent.img_seed == O.engine_seeds(2 * 4)[-1]                 # 2 epochs x 2 minibatches x 2 mini-epochs
