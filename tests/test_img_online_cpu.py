"""Camera-pair augmentation of the ONLINE student, host side: the seeded draws (``SyncTransform.draw_seeded``) against their
float64 restatement (tests/img_online_ref.py, which hashes through ``oracle.token_dropout``), the site table of
csrc/augment_seeded.h, ``apply_seeded``, the ``offline_train.img_augment_online`` key of ``ExtrinsicAdapt`` with its
default-off rule, the op's schema, fake kernel and refusals (they raise before any launch), and the condition the GPU tests'
seeds were chosen under.  No GPU."""
import math
import os
import re

import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import img_augment_ref as A
from tests import img_online_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaacgyminsertion_amd", "csrc")


def _U():
    from isaacgyminsertion_amd.algo.models.transformer import utils
    return utils


def _aug(H=54, W=96, patch=16, noise=0.0, masking=0.0, rot=0.0, crop=None):
    ch, cw = crop or (H, W)
    return _U().define_img_transforms(H, W, ch, cw, patch, noise, masking, rot)[3]


def test_names_through_both_import_paths():
    U = _U()
    import algo.ext_adapt.ext_adapt as shim_e
    import algo.models.transformer.utils as shim_u
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    assert shim_u.SyncTransform is U.SyncTransform is ext_adapt.SyncTransform is shim_e.SyncTransform
    assert shim_u.define_img_transforms is U.define_img_transforms
    for name in ("draw_seeded", "apply_seeded", "fused_seeded"):
        assert callable(getattr(U.SyncTransform, name))
    assert hasattr(ext_adapt.ExtrinsicAdapt, "_make_img_augment")
    assert "image_pair_augment_seeded" in ops.OP_NAMES and hasattr(torch.ops.mi355ppo, "image_pair_augment_seeded")


def test_site_table_of_the_header_and_the_python_tables_agree_and_share_no_site():
    from isaacgyminsertion_amd import draws
    hdr = open(os.path.join(CSRC, "augment_seeded.h")).read()
    tbl = open(os.path.join(CSRC, "draws.h")).read()
    ours = {k: int(re.search(rf"IMG_SITE_{k} = (\d+)", tbl).group(1)) for k in ("ANGLE", "KEEP")}
    assert ours == {k: draws.SITES["IMG_SITE_" + k] for k in ours} == O.SITES == {"ANGLE": 29, "KEEP": 30}
    for k, v in ours.items():                                 # the comment table says the same
        assert re.search(rf"//\s+site {v}\b", hdr), k
    assert re.search(r"//\s+plane 0 \(0,1\)", hdr) and re.search(r"//\s+plane 1 \(2,3\)", hdr)
    pcl_sites = {int(v) for v in re.findall(r"PCL_SITE_\w+ = (\d+)", tbl)}
    pcl_planes = {int(v) for v in re.findall(r"PCL_PLANE_\w+ = (\d+)", tbl)}
    tac_sites = {int(v) for v in re.findall(r"TAC_SITE_\w+ = (\d+)", tbl)}
    assert pcl_sites == set(range(14, 23)) and pcl_planes == {3, 4, 5, 6} and tac_sites == set(range(23, 29))
    assert tac_sites == {v for k, v in draws.SITES.items() if k.startswith("TAC_SITE_")}
    gauss_sites = {2 * p + k for p in {0, 1, 2} | pcl_planes for k in (0, 1)}          # aug_gauss.h: sites 2p, 2p + 1
    assert gauss_sites == set(range(14)) and "2u * plane" in open(os.path.join(CSRC, "aug_gauss.h")).read()
    assert len(set(ours.values())) == 2 and not set(ours.values()) & (pcl_sites | tac_sites | gauss_sites)
    assert f"IMG_MAX_CELLS = {ops.IMG_AUG_MAX_CELLS};" in hdr and ops.IMG_AUG_MAX_CELLS == 8192
    assert "draw_threshold(masking_prob)" in hdr and "draw_unit(" in hdr
    for p in (0.0, 0.3, 0.5, 1.0):
        assert draws.threshold(p) == O.threshold(p)


@pytest.mark.parametrize("case", O.CASES + [O.MANY[1:]], ids=str)
@pytest.mark.parametrize("seed", O.SEEDS)
def test_draw_seeded_equals_the_restatement_exactly(case, seed):
    T, H, W, patch, rot = case
    B = O.MANY[0] if case == O.MANY[1:] else len(O.ROWS)
    aug = _aug(H, W, patch, 0.01, 0.3, rot)
    off, ang, keep, s = aug.draw_seeded(B, T, seed)
    o2, a2, k2 = O.draws(B, T, seed, H, W, patch, 0.3, rot)
    assert s == seed and off.dtype == torch.int32 and not off.any() and off.shape == (B, 2)
    assert ang.dtype == torch.float32 and ang.shape == (B, 2) and keep.dtype == torch.uint8
    assert torch.equal(ang.view(torch.int32), O.angle_bits(a2))                          # the bits
    assert torch.equal(keep, k2) and keep.shape == (B * T, H // patch, W // patch)
    assert ang.abs().max() <= math.radians(rot) * (1 + 1e-6) and (ang != 0).all()
    assert not torch.equal(ang[:, 0], ang[:, 1])                                          # depth and mask: their own angles


def test_the_angle_is_one_rounding_of_exact_operands():
    """2u - 1 is exact in fp32, so the kernel's one fp32 multiply by ``max_rad`` is the correctly rounded value of the exact
    product, which float64 holds without rounding (24 + 24 bits): the fp32 expression of the kernel = the draws."""
    n, seed, rot = 4096, O.SEEDS[1], 1.0
    aug = _aug(rot=rot)
    _off, ang, _keep, _s = aug.draw_seeded(n, 1, seed)
    k = torch.from_numpy((O._hash(seed, O.SITES["ANGLE"], 2 * n) >> 8).astype("int64"))
    t32 = 2.0 * (k.float() * 2.0 ** -24) - 1.0                 # the kernel's own fp32 expression (draw_unit)
    assert torch.equal(t32.double(), k.double() * 2.0 ** -23 - 1.0)                     # exact
    rad = torch.tensor(rot * math.pi / 180.0, dtype=torch.float64).float()              # formed in double, rounded once
    assert float(rad) == aug.max_rad == O.max_rad(rot)
    assert torch.equal(ang.reshape(-1), t32 * rad)                                       # one fp32 multiply
    assert torch.equal(ang.reshape(-1), (t32.double() * float(rad)).float())


def test_event_frequencies_over_twenty_thousand_draws():
    B, T, seed, p_mask, rot = 10240, 1, 31337, 0.3, 1.0        # 20,480 angles; 10,240 frames x 18 cells
    _off, ang, keep, _s = _aug(54, 96, 16, 0.0, p_mask, rot).draw_seeded(B, T, seed)
    n = ang.numel()
    assert n >= 20000 and keep.numel() == B * 18

    def within(count, total, p):
        return abs(count - total * p) <= 5 * math.sqrt(total * p * (1 - p))
    assert within(int(keep.sum()), keep.numel(), 1 - p_mask)
    for c in range(18):                                        # every cell of the grid by itself
        assert within(int(keep.reshape(B, 18)[:, c].sum()), B, 1 - p_mask), c
    # uniform in +-m: mean 0 with standard deviation m / sqrt(3 n); the gap between the largest of n draws and m is
    # (nearly) exponential with mean = standard deviation = 2 m / n, so mean + 5 standard deviations is 12 m / n
    m = math.radians(rot)
    for col in (ang[:, 0], ang[:, 1], ang.reshape(-1)):
        k = col.numel()
        assert abs(float(col.double().mean())) <= 5 * m / math.sqrt(3 * k)
        assert m - 12 * m / k <= float(col.max()) <= m * (1 + 1e-6) and -m * (1 + 1e-6) <= float(col.min()) <= -m + 12 * m / k
    assert abs(float(ang.double().var()) - m * m / 3) <= 5 * (m * m / 3) * math.sqrt(0.8 / n)   # var of x^2: (4/45) m^4
    # the two angles of a sample are independent: their correlation is within 5 / sqrt(B)
    assert abs(float(torch.corrcoef(ang.double().T)[0, 1])) <= 5 / math.sqrt(B)
    assert len({tuple(g.flatten().tolist()) for g in keep[:64]}) > 32


def test_two_seeds_differ_and_a_seed_repeats():
    aug = _aug(54, 96, 8, 0.01, 0.3, 1.0)
    a, b, c = aug.draw_seeded(300, 2, 7), aug.draw_seeded(300, 2, 7), aug.draw_seeded(300, 2, 8)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == 7
    assert all(not torch.equal(x, y) for x, y in zip(a[1:3], c[1:3]))
    hi = aug.draw_seeded(300, 2, 7 + (1 << 32))                # the seed's high word enters the hash
    assert all(not torch.equal(x, y) for x, y in zip(a[1:3], hi[1:3]))
    few = aug.draw_seeded(10, 2, 7)                            # sample b's draws do not depend on how many there are
    assert torch.equal(few[1], a[1][:10]) and torch.equal(few[2], a[2][:20])
    # T frames of a sample: one angle pair (B rows, not B*T), a keep grid per frame
    assert a[1].shape == (300, 2) and a[2].shape[0] == 600 and not torch.equal(a[2][0], a[2][1])


def test_a_stage_that_is_off_draws_nothing_and_the_generator_is_left_alone():
    cpu_state = torch.get_rng_state()
    base = _aug(17, 23, 4, 0.0, 0.0, 0.0)
    base.generator = torch.Generator().manual_seed(3)
    own = base.generator.get_state()
    off, ang, keep, s = base.draw_seeded(5, 2, O.SEEDS[0])
    assert not off.any() and not ang.any() and keep is None and s == O.SEEDS[0] and base.max_rad == 0.0
    x, y = O.arena(2, 17, 23, seed=1, rows=5).double(), O.arena(2, 17, 23, seed=2, rows=5).double()
    oi, os_ = base.apply_seeded(x, y, off, ang, keep, 0.0, s)
    assert torch.equal(oi, x) and torch.equal(os_, y)          # everything off: the input
    # rotation on: the keep grid stays off, and the other way round -- a stage's draws do not depend on the others
    rot = _aug(17, 23, 4, 0.0, 0.0, 10.0)
    both = _aug(17, 23, 4, 0.05, 0.3, 10.0)
    mask = _aug(17, 23, 4, 0.0, 0.3, 0.0)
    assert rot.draw_seeded(5, 2, 9)[2] is None and not mask.draw_seeded(5, 2, 9)[1].any()
    assert torch.equal(rot.draw_seeded(5, 2, 9)[1], both.draw_seeded(5, 2, 9)[1])
    assert torch.equal(mask.draw_seeded(5, 2, 9)[2], both.draw_seeded(5, 2, 9)[2])
    # a patch larger than the frame leaves no whole cell: nothing to mask
    assert _aug(17, 23, 32, 0.0, 0.3).draw_seeded(5, 2, 9)[2] is None
    # without noise the seed is not looked at
    assert all(torch.equal(p, q) for p, q in zip(base.apply_seeded(x, y, off, ang, None, 0.0, 1),
                                                 base.apply_seeded(x, y, off, ang, None, 0.0, 2)))
    both.generator = torch.Generator().manual_seed(3)
    o, a, k, s = both.draw_seeded(5, 2, 9)
    both.apply_seeded(x, y, o, a, k, 0.05, s)
    assert torch.equal(both.generator.get_state(), own) and torch.equal(base.generator.get_state(), own)
    assert torch.equal(torch.get_rng_state(), cpu_state)       # and torch's global generator stands where it stood


@pytest.mark.parametrize("present", ["both", "img", "seg"])
@pytest.mark.parametrize("case", O.CASES, ids=str)
def test_apply_seeded_in_float64_matches_the_restatement(case, present):
    T, H, W, patch, rot = case
    img = O.arena(T, H, W, seed=2).double() if present != "seg" else None
    seg = O.arena(T, H, W, seed=3).double() if present != "img" else None
    rows, seed = torch.tensor(O.ROWS[:4]), O.SEEDS[1]
    aug = _aug(H, W, patch, 0.05, 0.3, rot)
    off, ang, keep, s = aug.draw_seeded(4, T, seed)
    pick = lambda a: None if a is None else a.index_select(0, rows)    # noqa: E731
    yi, ys = aug.apply_seeded(pick(img), pick(seg), off, ang, keep, 0.05, s)
    ri, rs, band, _d = O.augment(img, seg, rows, seed, patch, 0.05, 0.3, rot)
    assert band.double().mean() <= O.TIE_SHARE_MAX
    for k, (y, r, x) in enumerate(((yi, ri, img), (ys, rs, seg))):
        if x is None:
            assert y is None and r is None
            continue
        assert y.dtype == torch.float64 and y.shape == r.shape == (4, T, 1, H, W)
        assert torch.where(band[k], torch.zeros_like(r), (y - r).abs()).max() <= 1e-12
        clean = O.augment(img, seg, rows, seed, patch, 0.0, 0.3, rot)[k]
        assert (r - clean).abs().max() > 0.05                  # the noise is there
    if present == "both":                                      # a tensor's result does not depend on the other's presence
        assert torch.equal(aug.apply_seeded(pick(img), None, off, ang, keep, 0.05, s)[0], yi)
        assert torch.equal(aug.apply_seeded(None, pick(seg), off, ang, keep, 0.05, s)[1], ys)
        gh, gw = H // patch, W // patch
        if gh * gw > 1:
            dropped = A.patch_mask(keep, H, W, patch).reshape(yi.shape) == 0
            assert dropped.any() and not yi[dropped].any() and ys[dropped].all()   # only the depth frames are masked


def test_apply_runs_in_fp32_and_is_what_it_was():
    """``apply`` keeps torch's own noise and its arithmetic: with noise off it equals ``apply_seeded``."""
    aug = _aug(17, 23, 4, 0.0, 0.3, 10.0)
    x, y = O.arena(2, 17, 23, seed=1, rows=5), O.arena(2, 17, 23, seed=2, rows=5)
    off, ang, keep, s = aug.draw_seeded(5, 2, 4)
    a, b = aug.apply(x, y, off, ang, keep, 0.0), aug.apply_seeded(x, y, off, ang, keep, 0.0, s)
    assert a[0].dtype == torch.float32 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.manual_seed(1)
    n1 = aug.apply(x, y, off, ang, keep, 0.1)
    torch.manual_seed(1)
    n2 = aug.apply(x, y, off, ang, keep, 0.1)
    assert torch.equal(n1[0], n2[0]) and not torch.equal(n1[0], a[0])                    # torch.randn, from the global stream


def test_tie_share_of_every_gpu_seed_is_at_most_a_tenth_of_a_percent():
    """A condition on the seeds of tests/test_gpu_img_online.py, from the restatement alone: they were chosen for it."""
    assert O.TIE_SHARE_MAX == 0.001 and A.TIE_EPS == 1e-4
    for _T, H, W, _patch, rot in O.CASES:
        for seed in O.SEEDS:
            assert O.tie_share(len(O.ROWS), seed, H, W, rot) <= O.TIE_SHARE_MAX, (H, W, rot, seed)
    B, _T, H, W, _patch, rot = O.MANY
    for seed in O.SEEDS:
        assert O.tie_share(B, seed, H, W, rot) <= O.TIE_SHARE_MAX, seed
    # the largest turn moves pixels at every size (else the rotation tests would compare copies; they check that some do)
    for _T, H, W, _patch, rot in O.CASES:
        assert (max(H, W) / 2) * math.sin(math.radians(rot)) > 0.5, (H, W, rot)
    # the trainer cases: minibatches of 8 rows, the seeds of two epochs of the private generator's stream
    E = O.ENGINE
    rows = E["envs"] * E["horizon"] // E["mini_epochs"]
    for seed in O.engine_seeds(2 * E["mini_epochs"] ** 2 + 2):
        assert O.tie_share(rows, seed, *E["hw"], E["rotation_deg"]) <= O.TIE_SHARE_MAX, seed


# ---- the trainer's key --------------------------------------------------------------------------------------------------
_ABSENT = object()


def _engine(img_info=True, seg_info=True, img_hw=(54, 96), **offline_keys):
    """An ``ExtrinsicAdapt`` on the host: everything but its optimizer (HIP only, not under test) is built."""
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu", obs_info=True, img_info=img_info, seg_info=seg_info)
    for k, v in offline_keys.items():
        if v is _ABSENT:
            cfg.offline_train.pop(k, None)
        else:
            cfg.offline_train[k] = v
    env = SyntheticInsertionEnv(8, device="cpu", img_hw=img_hw)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ext_adapt, "FlatAdam", lambda *a, **k: None)
        agent = ExtrinsicAdapt(env, None, cfg)
    return agent, env


def test_default_config_has_the_key_off():
    from isaacgyminsertion_amd.utils.config import default_config
    assert default_config(num_envs=8, horizon_length=4, rl_device="cpu").offline_train.img_augment_online == "off"


class _Stop(Exception):
    pass


def _step(agent, seen):
    def predict(student_dict, requires_grad):
        seen["img"], seen["seg"] = student_dict["img"], student_dict["seg"]
        raise _Stop
    agent.student.predict = predict
    with pytest.raises(_Stop):
        agent.update_step(0)


@pytest.mark.parametrize("key", [_ABSENT, "off"], ids=["absent", "off"])
def test_key_off_builds_todays_objects(monkeypatch, key):
    calls = []
    S = _U().SyncTransform
    monkeypatch.setattr(S, "fused_seeded", lambda self, *a, **k: calls.append(a))
    monkeypatch.setattr(S, "draw_seeded", lambda self, *a, **k: calls.append(a))
    agent, _env = _engine(img_augment_online=key)
    assert agent.img_augment is None and agent.img_seed is None and not calls
    # today's step: n_img / n_seg are among the prefetched keys, and the batch's own gathers are what predict is handed
    seen = {}

    class Batch(dict):
        rows = None

        def prefetch(self, keys):
            seen["keys"] = keys
    img, seg = torch.zeros(2, 1, 5184), torch.ones(2, 1, 5184)
    agent.storage = [Batch(n_img=img, n_seg=seg, n_student_obs=torch.zeros(2, 15), teacher_actions=torch.zeros(2, 6))]
    _step(agent, seen)
    assert seen["keys"] == ('n_student_obs', 'n_tactile', 'n_img', 'n_seg', 'n_pcl', 'teacher_actions')
    assert seen["img"] is img and seen["seg"] is seg and not calls and agent.img_seed is None


def test_key_fused_builds_the_train_transform_with_the_offline_keys():
    U = _U()
    agent, _env = _engine(img_augment_online="fused", img_gaussian_noise=0.02, img_masking_prob=0.25, img_patch_size=8,
                          img_rotation_deg=2.0)
    a = agent.img_augment
    assert type(a) is U.SyncTransform and a.training and tuple(a.size) == a.crop_size == (54, 96)
    assert (a.patch, a.noise_std, a.masking_prob, a.rotation_deg) == (8, 0.02, 0.25, 2.0)
    stock, _env = _engine(img_augment_online="fused")
    s = stock.img_augment
    assert (s.noise_std, s.masking_prob, s.rotation_deg) == (0.0, 0.0, 0.0) and s.is_identity
    # one seed per step from a private generator seeded cfg.seed (+ rank): the stream the GPU tests restate
    drawn = [int(torch.randint(0, 2 ** 63 - 1, (1,), generator=s.generator)) for _ in range(4)]
    assert drawn == O.engine_seeds(4) and len(set(drawn)) == 4
    # apart from the tactile generator
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv  # noqa: F401
    assert stock.tactile_augment is None
    for infos in (dict(img_info=True, seg_info=False), dict(img_info=False, seg_info=True)):
        one, _env = _engine(img_augment_online="fused", **infos)
        assert one.img_augment is not None


@pytest.mark.parametrize("infos", [(True, True), (False, True), (True, False)], ids=["both", "seg_info", "img_info"])
def test_update_step_under_fused_leaves_the_camera_keys_out_of_the_prefetch(monkeypatch, infos):
    img_info, seg_info = infos
    agent, _env = _engine(img_info=img_info, seg_info=seg_info, img_augment_online="fused")
    seen, S = {}, _U().SyncTransform

    def fused_seeded(self, img_arena2d, seg_arena2d, rows, seed, want_draws=False):
        seen["call"] = (img_arena2d, seg_arena2d, rows, seed)
        return (None if img_arena2d is None else torch.ones(2, 1, 1, 54, 96),
                None if seg_arena2d is None else torch.full((2, 1, 1, 54, 96), 2.0), None)
    monkeypatch.setattr(S, "fused_seeded", fused_seeded)

    class Batch(dict):
        rows = torch.tensor([5, 9])

        def prefetch(self, keys):
            seen["keys"] = keys
    agent.storage.__class__ = type("S", (agent.storage.__class__,), {"__getitem__": lambda self, i: Batch(
        n_student_obs=torch.zeros(2, 15), teacher_actions=torch.zeros(2, 6))})
    _step(agent, seen)
    assert seen["keys"] == ('n_student_obs', 'n_tactile', 'n_pcl', 'teacher_actions')
    img2d, seg2d, rows, seed = seen["call"]
    store = agent.storage.storage_dict
    assert ("n_img" in store) == img_info and ("n_seg" in store) == seg_info      # what ExtrinsicAdapt stores under each info
    for a2d, name in ((img2d, "n_img"), (seg2d, "n_seg")):
        if name in store:
            assert a2d.shape == (4 * 8, 5184) and a2d.data_ptr() == store[name].data_ptr()      # the arena, in place
        else:
            assert a2d is None
    assert rows is Batch.rows and seed == O.engine_seeds(1)[0] == agent.img_seed
    assert (seen["img"] is None) == (not img_info) and (seen["seg"] is None) == (not seg_info)
    if img_info:
        assert bool((seen["img"] == 1).all())
    if seg_info:
        assert bool((seen["seg"] == 2).all())


def test_both_online_keys_together_leave_all_three_out():
    agent, _env = _engine(img_augment_online="fused", tactile_augment_online="off")
    assert agent.img_augment is not None and agent.tactile_augment is None
    # with the tactile key too (built on an env that has tactile frames)
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu", obs_info=True, img_info=True, seg_info=True,
                         tactile_info=True)
    cfg.offline_train.img_augment_online = cfg.offline_train.tactile_augment_online = "fused"
    env = SyntheticInsertionEnv(8, device="cpu", img_hw=(54, 96), tactile_hw=(32, 64))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ext_adapt, "FlatAdam", lambda *a, **k: None)
        agent = ExtrinsicAdapt(env, None, cfg)
    assert agent.img_augment.generator is not agent.tactile_augment.generator
    seen = {}

    class Batch(dict):
        rows = torch.tensor([5, 9])

        def prefetch(self, keys):
            seen["keys"] = keys
            raise _Stop
    agent.storage.__class__ = type("S", (agent.storage.__class__,), {"__getitem__": lambda self, i: Batch()})
    with pytest.raises(_Stop):
        agent.update_step(0)
    assert seen["keys"] == ('n_student_obs', 'n_pcl', 'teacher_actions')


_NAME = "offline_train.img_augment_online"
KEY_REFUSALS = [            # section 4's five refusals under "fused", each with every way into it
    ("value", ValueError, _NAME + ": expected 'off' or 'fused'",
     [dict(img_augment_online=bad) for bad in ("Fused", "torch", "on", "", True, 1)]),
    ("no camera", ValueError, _NAME + ".*img_info or train.ppo.seg_info",
     [dict(img_info=False, seg_info=False, img_hw=None, img_augment_online="fused")]),
    ("img_type", NotImplementedError, _NAME + ".*img_type", [dict(img_augment_online="fused", img_type="rgb")]),
    ("crop", NotImplementedError, _NAME + ".*does not crop",
     [dict(img_augment_online="fused", img_crop_w=4), dict(img_augment_online="fused", img_crop_h=8)]),
    ("frame length", ValueError, _NAME + ".*stored frames of img_width \\* img_height",
     [dict(img_augment_online="fused", img_width=60), dict(img_augment_online="fused", img_height=104),
      dict(img_augment_online="fused", img_width=96, img_height=96), dict(img_augment_online="fused", img_hw=(17, 23)),
      dict(img_augment_online="fused", img_info=False, img_hw=(17, 23))]),
]


@pytest.mark.parametrize("what, exc, message, ways", KEY_REFUSALS, ids=[r[0] for r in KEY_REFUSALS])
def test_key_refusals(what, exc, message, ways):
    for kwargs in ways:
        with pytest.raises(exc, match=message):
            _engine(**kwargs)


def test_key_off_asks_for_nothing():
    assert len(KEY_REFUSALS) == 5
    agent, _env = _engine(img_info=False, seg_info=False, img_hw=None, img_augment_online="off")
    assert agent.img_augment is None


def test_the_global_generators_are_untouched():
    cpu_state = torch.get_rng_state()
    aug = _aug(17, 23, 4, 0.01, 0.3, 10.0)
    off, ang, keep, s = aug.draw_seeded(64, 1, 5)
    aug.apply_seeded(O.arena(1, 17, 23, rows=64), O.arena(1, 17, 23, rows=64), off, ang, keep, 0.01, s)
    assert torch.equal(torch.get_rng_state(), cpu_state)
    agent, _env = _engine(img_augment_online="fused")
    before = torch.get_rng_state()
    int(torch.randint(0, 2 ** 63 - 1, (1,), generator=agent.img_augment.generator))
    assert torch.equal(torch.get_rng_state(), before)
    # building the trainer with the key on draws what it draws with the key off
    torch.manual_seed(3)
    _engine(img_augment_online="off")
    off_state = torch.get_rng_state()
    torch.manual_seed(3)
    _engine(img_augment_online="fused")
    assert torch.equal(torch.get_rng_state(), off_state)


def test_fused_seeded_checks_its_arenas_before_any_launch():
    aug = _aug(17, 23, 4, 0.01, 0.3, 10.0)
    rows = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="at least one arena"):
        aug.fused_seeded(None, None, rows, 1)
    with pytest.raises(ValueError, match="arena2d"):
        aug.fused_seeded(torch.zeros(6, 1, 391), None, rows, 1)
    with pytest.raises(ValueError, match="arena2d"):
        aug.fused_seeded(None, torch.zeros(6, 392), rows, 1)
    with pytest.raises(ValueError, match="arena2d"):
        aug.fused_seeded(torch.zeros(6, 391), torch.zeros(6, 782), rows, 1)
    with pytest.raises(NotImplementedError, match="does not crop"):
        _aug(60, 104, crop=(54, 96)).fused_seeded(torch.zeros(6, 6240), None, rows, 1)
    # evaluation is the gather
    x = torch.rand(6, 2 * 391)
    i, s, d = aug.eval().fused_seeded(x, None, torch.tensor([4, 1]), 1, want_draws=True)
    assert s is None and d is None and torch.equal(i, x[[4, 1]].reshape(2, 2, 1, 17, 23))
    aug.train()
    with pytest.raises(RuntimeError, match="expected a HIP"):      # training on host tensors: the op, which has no CPU path
        aug.fused_seeded(x, None, torch.tensor([4, 1]), 1)
    # more cells than the kernel's grid holds: the same draws in torch ops, on the host too
    big = _aug(96, 96, 1, 0.01, 0.3, 3.0)
    xb, yb = torch.rand(3, 9216), torch.rand(3, 9216)
    rb = torch.tensor([2, 0])
    i, s, d = big.fused_seeded(xb, yb, rb, 11, want_draws=True)
    o, a, k, sd = big.draw_seeded(2, 1, 11)
    wi, ws = big.apply_seeded(xb[rb].reshape(2, 1, 1, 96, 96), yb[rb].reshape(2, 1, 1, 96, 96), o, a, k, 0.01, sd)
    assert torch.equal(i, wi) and torch.equal(s, ws) and torch.equal(d, O.angle_bits(a)) and d.dtype == torch.int32


# ---- the op --------------------------------------------------------------------------------------------------------------
def _op_args(B=3, R_=6, T=2, h=17, w=23):
    return dict(img_arena=torch.zeros(R_, T * h * w), seg_arena=torch.zeros(R_, T * h * w),
                rows=torch.zeros(B, dtype=torch.int64), T=T, h=h, w=w, patch=4, noise_std=0.0, masking_prob=0.3,
                max_rad=0.01, seed=1, want_draws=True)


SCHEMA = ("mi355ppo::image_pair_augment_seeded(Tensor? img_arena, Tensor? seg_arena, Tensor rows, int T, int h, int w, "
          "int patch, float noise_std, float masking_prob, float max_rad, int seed, bool want_draws) -> "
          "(Tensor?, Tensor?, Tensor?)")


def test_op_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.mi355ppo.image_pair_augment_seeded
    assert str(op.default._schema) == SCHEMA
    with FakeTensorMode():
        i, s, d = op(*_op_args().values())
        assert i.shape == s.shape == (3, 2, 1, 17, 23) and i.dtype == s.dtype == torch.float32
        assert d.shape == (3, 2) and d.dtype == torch.int32
        i, s, d = op(*{**_op_args(), "img_arena": None, "want_draws": False}.values())
        assert i is None and s.shape == (3, 2, 1, 17, 23) and d is None
        i, s, d = op(*{**_op_args(), "seg_arena": None}.values())
        assert s is None and i.shape == (3, 2, 1, 17, 23) and d.shape == (3, 2)


def test_c_abi_python_binding_and_cpp_registration_agree():
    from isaacgyminsertion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "igi_ppo.h")).read()
    capi = open(os.path.join(CSRC, "igi_capi.hip")).read()
    cpp = open(os.path.join(CSRC, "torch_ops.cpp")).read()
    assert "igi_image_pair_augment_seeded" in _lib.exported_symbols()
    pat = r"^int igi_image_pair_augment_seeded\((.*?)\)"
    assert re.search(pat, hdr, re.M | re.S) and re.search(pat, capi, re.M | re.S)
    decl = re.search(pat + ";", hdr, re.M | re.S).group(1)
    assert re.sub(r"\s+", " ", decl) == re.sub(r"\s+", " ", re.search(pat + r" \{", capi, re.M | re.S).group(1))
    assert len(_lib._EXPORTS["igi_image_pair_augment_seeded"][1]) == len(decl.split(",")) == 17
    assert "double masking_prob" in decl and "float max_rad" in decl and "uint64_t seed" in decl and "int32_t* draws" in decl
    schema = SCHEMA.replace("mi355ppo::", "")
    assert f'm.def("{schema}");' in cpp and 'm.impl("image_pair_augment_seeded", image_pair_augment_seeded);' in cpp
    kern = open(os.path.join(CSRC, "augment_seeded.h")).read()
    assert "void k_image_pair_augment_seeded(" in kern and "IGI_E_UNSUPPORTED" in kern and '#include "augment_seeded.h"' in capi
    # the kernel's own refusals, read from its launch function: an output that is an arena, frames above 2^24 pixels
    assert "out_img == img || out_img == seg" in kern and "out_seg == img || out_seg == seg" in kern
    assert "(long long)hs * ws > (1ll << 24)" in kern
    # the new header is among the sources the build hash covers
    import __graft_entry__ as G
    assert "augment_seeded.h" in [os.path.basename(p) for p in G._sources()]


_W = 2 * 17 * 23
OP_REFUSALS = [
    (dict(img_arena=None, seg_arena=None), "img_arena / seg_arena: expected at least one arena"),        # both absent
    (dict(img_arena=torch.zeros(6, _W, dtype=torch.float64)), "img_arena: expected dtype"),                # not fp32
    (dict(seg_arena=torch.zeros(6, _W, dtype=torch.float16)), "seg_arena: expected dtype"),
    (dict(img_arena=torch.zeros(_W, 6).t()), "img_arena: expected a contiguous"),                          # not contiguous
    (dict(seg_arena=torch.zeros(6, 2 * _W)[:, ::2]), "seg_arena: expected a contiguous"),
    (dict(img_arena=torch.zeros(6, 2, 1, 17, 23)), "img_arena: expected 2 dimensions"),
    (dict(img_arena=torch.zeros(6, _W + 1)), r"img_arena: expected \(R, T\*h\*w = 782\)"),                 # a width that is not T*h*w
    (dict(seg_arena=torch.zeros(6, 17 * 23)), r"seg_arena: expected \(R, T\*h\*w = 782\)"),
    (dict(img_arena=None, seg_arena=torch.zeros(0, _W)), r"seg_arena: expected \(R, T\*h\*w = 782\) non-empty"),
    (dict(seg_arena=torch.zeros(5, _W)), "seg_arena: expected img_arena's shape"),
    (dict(T=0), "T / h / w: expected >= 1"),
    (dict(rows=torch.zeros(3, dtype=torch.int32)), "rows: expected dtype"),                                # rows not int64
    (dict(rows=torch.zeros(3, 1, dtype=torch.int64)), "rows: expected 1 dimensions"),
    (dict(rows=torch.zeros(6, dtype=torch.int64)[::2]), "rows: expected a contiguous"),
    (dict(masking_prob=1.5), r"masking_prob: expected a value in \[0, 1\]"),                               # probabilities
    (dict(masking_prob=-0.1), r"masking_prob: expected a value in \[0, 1\]"),
    (dict(masking_prob=float("nan")), r"masking_prob: expected a value in \[0, 1\]"),
    (dict(patch=0), "patch: expected >= 1"),                                                               # patch < 1, masking on
    (dict(noise_std=-0.001), "noise_std: expected >= 0"),                                                  # negative / NaN
    (dict(noise_std=float("nan")), "noise_std: expected >= 0"),
    (dict(max_rad=-0.1), "max_rad: expected >= 0"),
    (dict(max_rad=float("nan")), "max_rad: expected >= 0"),
    (dict(), "expected a HIP"),                                   # everything else right, CPU tensors: no CPU path
    (dict(img_arena=None), "expected a HIP"),
    (dict(seg_arena=None), "expected a HIP"),
]


@pytest.mark.parametrize("change, message", OP_REFUSALS)
def test_op_refuses_bad_arguments(change, message):
    args = {**_op_args(), **change}
    with pytest.raises(RuntimeError, match=message):
        torch.ops.mi355ppo.image_pair_augment_seeded(*args.values())


def test_patch_zero_without_masking_is_not_looked_at():
    with pytest.raises(RuntimeError, match="expected a HIP"):     # past every argument check: refused for the device alone
        torch.ops.mi355ppo.image_pair_augment_seeded(*{**_op_args(), "masking_prob": 0.0, "patch": 0}.values())


def test_the_refusals_are_counted():
    """The op's twenty-five cases cover nine of the kinds the op refuses by name: both arenas absent, CPU tensors, dtype,
    contiguity, width, rows, probabilities, patch, noise_std (and max_rad).  The tenth, an output that is an arena, cannot be
    reached through the op, which allocates its outputs: the C entry refuses it (tests/test_gpu_img_online.py)."""
    assert len(OP_REFUSALS) == 25 and len({m for _c, m in OP_REFUSALS}) == 19 and len(KEY_REFUSALS) == 5
