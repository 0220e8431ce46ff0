"""Tactile augmentation of the ONLINE student, host side: the seeded draws (``TactileAugment.draw_seeded``) against their
float64 restatement (tests/tactile_online_ref.py, which hashes through ``oracle.token_dropout``), the site table of
csrc/tactile_augment_seeded.h, the ``offline_train.tactile_augment_online`` key of ``ExtrinsicAdapt`` with its default-off
rule, the op's schema, fake kernel and refusals (they raise before any launch), and the condition the GPU tests' seeds were
chosen under.  No GPU."""
import math
import os
import re

import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import tactile_augment_ref as R
from tests import tactile_online_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaacgyminsertion_amd", "csrc")


def _U():
    from isaacgyminsertion_amd.algo.models.transformer import utils
    return utils


def _aug(H=32, W=64, patch=16, noise=0.0, masking=0.0, train=True):
    return _U().TactileAugment((H, W), (H, W), patch, noise, masking, train=train)


def test_names_through_both_import_paths():
    U = _U()
    import algo.ext_adapt.ext_adapt as shim_e
    import algo.models.transformer.utils as shim_u
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    from isaacgyminsertion_amd.algo.ppo.experience import _LazyMinibatch
    assert shim_u.TactileAugment is U.TactileAugment is ext_adapt.TactileAugment is shim_e.TactileAugment
    assert shim_u.define_tactile_transforms is U.define_tactile_transforms
    for name in ("draw_seeded", "fused_seeded"):
        assert callable(getattr(U.TactileAugment, name))
    assert hasattr(ext_adapt.ExtrinsicAdapt, "_make_tactile_augment")
    assert "tactile_augment_seeded" in ops.OP_NAMES and hasattr(torch.ops.mi355ppo, "tactile_augment_seeded")
    flat = torch.tensor([3, 1, 2])
    mb = _LazyMinibatch({"a": torch.zeros(2, 2, 1)}, flat, 4)
    assert mb.rows is flat
    with pytest.raises(AttributeError):
        mb.rows = flat                                        # read-only


def test_site_table_of_the_header_and_the_python_tables_agree_and_share_no_site():
    U = _U()
    from isaacgyminsertion_amd import draws
    hdr = open(os.path.join(CSRC, "tactile_augment_seeded.h")).read()
    tbl = open(os.path.join(CSRC, "draws.h")).read()
    names = dict(JITTER="JITTER", BRIGHT="BRIGHT", CONTRAST="CONTRAST", ROTATE="ROTATE", ANGLE="ANGLE", KEEP="KEEP")
    ours = {k: int(re.search(rf"TAC_SITE_{v} = (\d+)", tbl).group(1)) for k, v in names.items()}
    assert ours == {k: draws.SITES["TAC_SITE_" + k] for k in ours} == O.SITES
    assert ours == dict(JITTER=23, BRIGHT=24, CONTRAST=25, ROTATE=26, ANGLE=27, KEEP=28)
    for k, v in ours.items():                                 # the comment table says the same
        assert re.search(rf"//\s+site {v}\b", hdr), k
    pcl_sites = {int(v) for v in re.findall(r"PCL_SITE_\w+ = (\d+)", tbl)}
    pcl_planes = {int(v) for v in re.findall(r"PCL_PLANE_\w+ = (\d+)", tbl)}
    assert pcl_sites == set(range(14, 23)) and pcl_planes == {3, 4, 5, 6}
    gauss_sites = {2 * p + k for p in {0, 1, 2} | pcl_planes for k in (0, 1)}          # aug_gauss.h: sites 2p, 2p + 1
    assert gauss_sites == set(range(14))
    assert int(re.search(r"TAC_NOISE_PLANE = (\d+)", tbl).group(1)) == 2
    assert "2u * plane" in open(os.path.join(CSRC, "aug_gauss.h")).read()
    assert R.NOISE_PLANE == draws.PLANES["TAC_NOISE_PLANE"] == 2
    assert len(set(ours.values())) == 6 and not set(ours.values()) & (pcl_sites | gauss_sites)
    # the probabilities and amplitudes of the class are the restatement's and the header's
    T = U.TactileAugment
    assert (T.JITTER_P, T.ROTATE_P, T.JITTER, T.ROTATE_DEG) == (O.JITTER_P, O.ROTATE_P, O.JITTER, O.ROTATE_DEG)
    assert "draw_threshold(0.3)" in hdr and "draw_threshold(0.5)" in hdr and "TAC_JITTER = 0.1f" in hdr
    assert "3.0 * 3.141592653589793 / 180.0" in hdr and "__fmaf_rn" in hdr
    for p in (0.0, 0.3, 0.5, 0.75, 1.0):
        assert draws.threshold(p) == O.threshold(p)
    assert O.threshold(1.0) == 2 ** 32


@pytest.mark.parametrize("case", O.CASES + [O.MANY[1:]], ids=str)
@pytest.mark.parametrize("seed", O.SEEDS)
def test_draw_seeded_equals_the_restatement_exactly(case, seed):
    T, Fg, H, W, patch = case
    n = (O.MANY[0] if (T, Fg) == (1, 1) else len(O.ROWS)) * T * Fg
    aug = _aug(H, W, patch, 0.01, 0.3)
    off, jit, ang, keep, s = aug.draw_seeded(n, seed)
    o2, j2, a2, k2 = O.draws(n, seed, H, W, patch, 0.3)
    assert s == seed and off.dtype == torch.int32 and not off.any() and off.shape == (n, 2)
    assert jit.dtype == torch.float32 and ang.dtype == torch.float32 and keep.dtype == torch.uint8
    assert torch.equal(jit, j2) and torch.equal(ang, a2) and torch.equal(keep, k2) and keep.shape == (n, H // patch, W // patch)
    assert torch.equal(aug.pack(off, jit, ang), O.packed(o2, j2, a2))
    on, turn = jit[:, 0] != 0, ang != 0
    assert (jit[~on, 1:] == 1).all() and (jit[on, 1:] >= 0.9).all() and (jit[on, 1:] <= 1.1).all()
    assert ang.abs().max() <= math.radians(3.0) + 1e-9 and on.any() and turn.any() and not on.all() and not turn.all()


def test_the_factors_are_one_rounding_of_exact_operands():
    """2u - 1 is exact in fp32, so the kernel's fmaf(2u - 1, 0.1f, 1) is the correctly rounded value of the exact sum, which
    float64 holds without rounding: fp32 fma arithmetic (emulated through the exact float64 sum) = the draws."""
    n, seed = 4096, O.SEEDS[1]
    _off, jit, ang, _keep, _s = _aug().draw_seeded(n, seed)
    k = torch.from_numpy((O._hash(seed, O.SITES["BRIGHT"], n) >> 8).astype("int64"))
    t32 = 2.0 * (k.float() * 2.0 ** -24) - 1.0                 # the kernel's own fp32 expression
    assert torch.equal(t32.double(), k.double() * 2.0 ** -23 - 1.0)                     # exact
    exact = t32.double() * float(torch.tensor(0.1, dtype=torch.float32)) + 1.0            # 48-bit product + 1: 51 bits
    on = jit[:, 0] != 0
    assert torch.equal(jit[on, 1], exact.float()[on]) and on.sum() > 1000
    k = torch.from_numpy((O._hash(seed, O.SITES["ANGLE"], n) >> 8).astype("int64"))
    rad = torch.tensor(3.0 * math.pi / 180.0, dtype=torch.float64).float()
    want = ((2.0 * (k.float() * 2.0 ** -24) - 1.0) * rad)                                 # one fp32 multiply
    assert torch.equal(ang[ang != 0], want[ang != 0])


def test_event_frequencies_over_24576_images():
    n, seed, p_mask = 24576, 31337, 0.3                        # 8192 samples x 3 fingers: the online minibatch
    _off, jit, ang, keep, _s = _aug(32, 64, 16, 0.0, p_mask).draw_seeded(n, seed)

    def within(count, total, p):
        return abs(count - total * p) <= 5 * math.sqrt(total * p * (1 - p))
    on, turn = jit[:, 0] != 0, ang != 0
    assert within(int(on.sum()), n, 0.3) and within(int(turn.sum()), n, 0.5)
    assert within(int(keep.sum()), keep.numel(), 1 - p_mask) and keep.numel() == n * 8
    assert within(int((on & turn).sum()), n, 0.15)             # independent flags
    # the factors and the angle fill their ranges, on both sides
    assert jit[on, 1].min() < 0.901 and jit[on, 1].max() > 1.099 and jit[on, 2].min() < 0.901 and jit[on, 2].max() > 1.099
    assert not torch.equal(jit[on, 1], jit[on, 2])
    lim = math.radians(3.0)
    assert ang.min() < -0.99 * lim and ang.max() > 0.99 * lim
    assert abs(float(jit[on, 1].double().mean()) - 1.0) < 5 * 0.1 / math.sqrt(3 * int(on.sum()))
    assert not torch.equal(keep[0], keep[1]) and len({tuple(k.flatten().tolist()) for k in keep[:64]}) > 32


def test_two_seeds_differ_and_a_seed_repeats():
    aug = _aug(32, 64, 8, 0.01, 0.3)
    a, b, c = aug.draw_seeded(300, 7), aug.draw_seeded(300, 7), aug.draw_seeded(300, 8)
    assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] == 7
    assert all(not torch.equal(x, y) for x, y in zip(a[1:4], c[1:4]))
    hi = aug.draw_seeded(300, 7 + (1 << 32))                   # the seed's high word enters the hash
    assert all(not torch.equal(x, y) for x, y in zip(a[1:4], hi[1:4]))
    # image i's draws do not depend on how many images there are
    few = aug.draw_seeded(10, 7)
    assert torch.equal(few[1], a[1][:10]) and torch.equal(few[2], a[2][:10])


def test_a_stage_that_is_off_draws_nothing_that_changes_the_output():
    x = O.arena(2, 3, 32, 64, seed=1, rows=3).double()
    n, seed = 18, O.SEEDS[0]
    base = _aug(32, 64, 16, 0.0, 0.0)
    off, jit, ang, keep, s = base.draw_seeded(n, seed)
    assert keep is None
    y = base.apply(x, off, jit, ang, keep, 0.0, s)
    # masking on: the same jitter and angles; only the masked cells differ
    m = _aug(32, 64, 16, 0.0, 0.3)
    _o, jit_m, ang_m, keep_m, _s = m.draw_seeded(n, seed)
    assert torch.equal(jit_m, jit) and torch.equal(ang_m, ang) and keep_m is not None
    ym = m.apply(x, off, jit_m, ang_m, keep_m, 0.0, s)
    assert torch.equal(ym, y * R.patch_mask(keep_m, 32, 64, 16).reshape(y.shape))
    # noise on: the same draws, and without it the seed is not looked at
    nz = _aug(32, 64, 16, 0.01, 0.0)
    assert all(torch.equal(p, q) for p, q in zip(nz.draw_seeded(n, seed)[1:3], (jit, ang)))
    assert torch.equal(base.apply(x, off, jit, ang, None, 0.0, seed + 1), y)
    # images with both flags off are the input, bit for bit
    still = ((jit[:, 0] == 0) & (ang == 0)).reshape(3, 2, 3)
    assert still.any() and torch.equal(y[still], x[still])
    # a patch larger than the frame leaves no whole cell: nothing to mask
    assert _aug(9, 13, 16, 0.0, 0.3).draw_seeded(n, seed)[3] is None
    # evaluation: nothing drawn at all
    off, jit, ang, keep, s = _aug(32, 64, 16, 0.01, 0.3, train=False).draw_seeded(n, seed)
    assert not off.any() and not jit[:, 0].any() and (jit[:, 1:] == 1).all() and not ang.any() and keep is None and s == 0


@pytest.mark.parametrize("case", O.CASES[:4], ids=str)
def test_apply_with_seeded_draws_in_float64_matches_the_restatement(case):
    T, Fg, H, W, patch = case
    arena = O.arena(T, Fg, H, W, seed=2).double()
    rows = torch.tensor(O.ROWS[:4])
    seed = O.SEEDS[1]
    aug = _aug(H, W, patch, 0.05, 0.3)
    off, jit, ang, keep, s = aug.draw_seeded(rows.numel() * T * Fg, seed)
    y = aug.apply(arena.index_select(0, rows), off, jit, ang, keep, 0.05, s)
    ref, band, _d = O.augment(arena, rows, seed, patch, 0.05, 0.3)
    assert y.dtype == torch.float64 and y.shape == ref.shape == (4, T, Fg, 1, H, W)
    assert band.double().mean() <= O.TIE_SHARE_MAX
    assert torch.where(band, torch.zeros_like(ref), (y - ref).abs()).max() <= 1e-12
    clean, _b, _d = O.augment(arena, rows, seed, patch, 0.0, 0.3)
    assert (ref - clean).abs().max() > 0.05                    # the noise is there


def test_tie_share_of_every_gpu_seed_is_at_most_a_tenth_of_a_percent():
    """A condition on the seeds of tests/test_gpu_tactile_online.py, from the restatement alone: they were chosen for it."""
    assert O.TIE_SHARE_MAX == 0.001 and R.TIE_EPS == 1e-4
    for T, Fg, H, W, _patch in O.CASES:
        for seed in O.SEEDS:
            assert O.tie_share(len(O.ROWS) * T * Fg, seed, H, W) <= O.TIE_SHARE_MAX, (H, W, seed)
    B, T, Fg, H, W, _patch = O.MANY
    for seed in O.SEEDS:
        assert O.tie_share(B * T * Fg, seed, H, W) <= O.TIE_SHARE_MAX, seed
    _off, jit, ang, _keep = O.draws(1, O.EDGE_SEED, 64, 128, 16, 0.0)
    assert jit[0, 0] != 0 and ang[0] != 0 and O.tie_share(1, O.EDGE_SEED, 64, 128) <= O.TIE_SHARE_MAX
    # the trainer cases: minibatches of 8 rows x 3 fingers, the seeds of two epochs of the private generator's stream
    E = O.ENGINE
    rows = E["envs"] * E["horizon"] // E["mini_epochs"]
    for seed in O.engine_seeds(2 * E["mini_epochs"] ** 2):
        assert O.tie_share(rows * 3, seed, 32, 64) <= O.TIE_SHARE_MAX, seed


# ---- the trainer's key --------------------------------------------------------------------------------------------------
_ABSENT = object()


def _engine(tactile_info=True, **offline_keys):
    """An ``ExtrinsicAdapt`` on the host: everything but its optimizer (HIP only, not under test) is built."""
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu", obs_info=True, tactile_info=tactile_info)
    for k, v in offline_keys.items():
        if v is _ABSENT:
            cfg.offline_train.pop(k, None)
        else:
            cfg.offline_train[k] = v
    env = SyntheticInsertionEnv(8, device="cpu", tactile_hw=(32, 64) if tactile_info else None)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ext_adapt, "FlatAdam", lambda *a, **k: None)
        agent = ExtrinsicAdapt(env, None, cfg)
    return agent, env


def test_default_config_has_the_key_off():
    from isaacgyminsertion_amd.utils.config import default_config
    assert default_config(num_envs=8, horizon_length=4, rl_device="cpu").offline_train.tactile_augment_online == "off"


@pytest.mark.parametrize("key", [_ABSENT, "off"], ids=["absent", "off"])
def test_key_off_builds_todays_objects(monkeypatch, key):
    calls = []
    T = _U().TactileAugment
    monkeypatch.setattr(T, "fused_seeded", lambda self, *a, **k: calls.append(a))
    monkeypatch.setattr(T, "draw_seeded", lambda self, *a, **k: calls.append(a))
    agent, _env = _engine(tactile_augment_online=key)
    assert agent.tactile_augment is None and agent.tactile_seed is None and not calls
    # today's step: n_tactile is one of the prefetched keys, and the batch's own gather is what predict is handed
    seen = {}

    class Batch(dict):
        rows = None

        def prefetch(self, keys):
            seen["keys"] = keys

    class Stop(Exception):
        pass

    def predict(student_dict, requires_grad):
        seen["tactile"] = student_dict["tactile"]
        raise Stop
    tac = torch.zeros(2, 1, 3, 2048)
    agent.storage = [Batch(n_tactile=tac, n_student_obs=torch.zeros(2, 18), teacher_actions=torch.zeros(2, 6))]
    agent.student.predict = predict
    with pytest.raises(Stop):
        agent.update_step(0)
    assert seen["keys"] == ('n_student_obs', 'n_tactile', 'n_img', 'n_seg', 'n_pcl', 'teacher_actions')
    assert seen["tactile"] is tac and not calls


def test_key_fused_builds_the_train_transform_with_the_reference_keys():
    U = _U()
    agent, _env = _engine(tactile_augment_online="fused", tactile_gaussian_noise=0.002, tactile_masking_prob=0.25,
                          tactile_patch_size=8)
    a = agent.tactile_augment
    assert isinstance(a, U.TactileAugment) and a.training and a.size == a.crop_size == (32, 64)
    assert (a.patch, a.noise_std, a.masking_prob) == (8, 0.002, 0.25)
    stock, _env = _engine(tactile_augment_online="fused")
    s = stock.tactile_augment
    assert (s.patch, s.noise_std, s.masking_prob) == (16, 0.001, 0.0)
    # one seed per step from a private generator seeded cfg.seed (+ rank): the stream the GPU tests restate
    drawn = [int(torch.randint(0, 2 ** 63 - 1, (1,), generator=s.generator)) for _ in range(4)]
    assert drawn == O.engine_seeds(4) and len(set(drawn)) == 4


def test_update_step_under_fused_leaves_n_tactile_out_of_the_prefetch(monkeypatch):
    agent, _env = _engine(tactile_augment_online="fused")
    seen, T = {}, _U().TactileAugment

    def fused_seeded(self, arena2d, rows, seed, want_draws=False, fingers=3):
        seen["call"] = (arena2d, rows, seed)
        return torch.ones(2, 1, 3, 1, 32, 64), None
    monkeypatch.setattr(T, "fused_seeded", fused_seeded)

    class Batch(dict):
        rows = torch.tensor([5, 9])

        def prefetch(self, keys):
            seen["keys"] = keys

    class Stop(Exception):
        pass

    def predict(student_dict, requires_grad):
        seen["tactile"] = student_dict["tactile"]
        raise Stop
    agent.storage.__class__ = type("S", (agent.storage.__class__,), {"__getitem__": lambda self, i: Batch(
        n_student_obs=torch.zeros(2, 18), teacher_actions=torch.zeros(2, 6))})
    agent.student.predict = predict
    with pytest.raises(Stop):
        agent.update_step(0)
    assert seen["keys"] == ('n_student_obs', 'n_img', 'n_seg', 'n_pcl', 'teacher_actions')
    arena2d, rows, seed = seen["call"]
    store = agent.storage.storage_dict["n_tactile"]
    assert arena2d.shape == (4 * 8, 3 * 2048) and arena2d.data_ptr() == store.data_ptr()       # the arena, in place
    assert rows is Batch.rows and seed == O.engine_seeds(1)[0] == agent.tactile_seed
    assert seen["tactile"].shape == (2, 1, 3, 1, 32, 64) and bool((seen["tactile"] == 1).all())


def test_key_refusals():
    name = "offline_train.tactile_augment_online"
    for bad in ("Fused", "torch", "on", "", True, 1):
        with pytest.raises(ValueError, match=name):
            _engine(tactile_augment_online=bad)
    with pytest.raises(ValueError, match=name + ".*tactile_info"):
        _engine(tactile_info=False, tactile_augment_online="fused")
    with pytest.raises(NotImplementedError, match=name + ".*tactile_type"):
        _engine(tactile_augment_online="fused", tactile_type="rgb")
    for crop in (dict(tactile_crop_w=4), dict(tactile_crop_h=8)):
        with pytest.raises(NotImplementedError, match=name + ".*does not crop"):
            _engine(tactile_augment_online="fused", **crop)
    _engine(tactile_info=False, tactile_augment_online="off")     # off asks for nothing


def test_the_global_generators_are_untouched():
    cpu_state = torch.get_rng_state()
    aug = _aug(32, 64, 16, 0.01, 0.3)
    off, jit, ang, keep, s = aug.draw_seeded(64, 5)
    aug.apply(O.arena(1, 1, 32, 64, rows=64), off, jit, ang, keep, 0.01, s)
    assert torch.equal(torch.get_rng_state(), cpu_state)
    agent, _env = _engine(tactile_augment_online="fused")
    before = torch.get_rng_state()
    int(torch.randint(0, 2 ** 63 - 1, (1,), generator=agent.tactile_augment.generator))
    assert torch.equal(torch.get_rng_state(), before)
    # building the trainer with the key on draws what it draws with the key off
    torch.manual_seed(3)
    _engine(tactile_augment_online="off")
    off_state = torch.get_rng_state()
    torch.manual_seed(3)
    _engine(tactile_augment_online="fused")
    assert torch.equal(torch.get_rng_state(), off_state)


def test_fused_seeded_checks_its_arena_before_any_launch():
    aug = _aug()
    rows = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="arena2d"):
        aug.fused_seeded(torch.zeros(6, 1, 3, 2048), rows, 1)
    with pytest.raises(ValueError, match="arena2d"):
        aug.fused_seeded(torch.zeros(6, 3 * 2048 + 1), rows, 1)
    with pytest.raises(NotImplementedError, match="does not crop"):
        _U().TactileAugment((32, 64), (28, 56)).fused_seeded(torch.zeros(6, 3 * 2048), rows, 1)
    # evaluation is the gather
    x = torch.rand(6, 2 * 3 * 2048)
    y, d = _aug(train=False).fused_seeded(x, torch.tensor([4, 1]), 1, want_draws=True)
    assert d is None and torch.equal(y, x[[4, 1]].reshape(2, 2, 3, 1, 32, 64))
    with pytest.raises(RuntimeError, match="expected a HIP"):      # training on host tensors: the op, which has no CPU path
        aug.fused_seeded(x, torch.tensor([4, 1]), 1)


# ---- the op --------------------------------------------------------------------------------------------------------------
def _op_args(B=3, R_=6, T=2, Fg=3, Hs=9, Ws=13):
    return dict(arena=torch.zeros(R_, T, Fg, 1, Hs, Ws), rows=torch.zeros(B, dtype=torch.int64), out_h=9, out_w=13, patch=4,
                noise_std=0.0, masking_prob=0.3, seed=1, want_draws=True)


SCHEMA = ("mi355ppo::tactile_augment_seeded(Tensor arena, Tensor rows, int out_h, int out_w, int patch, float noise_std, "
          "float masking_prob, int seed, bool want_draws) -> (Tensor, Tensor?)")


def test_op_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mi355ppo.tactile_augment_seeded.default._schema) == SCHEMA
    with FakeTensorMode():
        y, d = torch.ops.mi355ppo.tactile_augment_seeded(*_op_args().values())
        assert y.shape == (3, 2, 3, 1, 9, 13) and y.dtype == torch.float32
        assert d.shape == (18, ops.TACTILE_AUG_WORDS) and d.dtype == torch.int32
        y, d = torch.ops.mi355ppo.tactile_augment_seeded(*{**_op_args(), "want_draws": False, "out_h": 5, "out_w": 6}.values())
        assert y.shape == (3, 2, 3, 1, 5, 6) and d is None


def test_c_abi_python_binding_and_cpp_registration_agree():
    from isaacgyminsertion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "igi_ppo.h")).read()
    capi = open(os.path.join(CSRC, "igi_capi.hip")).read()
    cpp = open(os.path.join(CSRC, "torch_ops.cpp")).read()
    assert "igi_tactile_augment_seeded" in _lib.exported_symbols()
    pat = r"^int igi_tactile_augment_seeded\((.*?)\)"
    assert re.search(pat, hdr, re.M | re.S) and re.search(pat, capi, re.M | re.S)
    decl = re.search(pat + ";", hdr, re.M | re.S).group(1)
    assert re.sub(r"\s+", " ", decl) == re.sub(r"\s+", " ", re.search(pat + r" \{", capi, re.M | re.S).group(1))
    assert len(_lib._EXPORTS["igi_tactile_augment_seeded"][1]) == len(decl.split(",")) == 16
    assert "double masking_prob" in decl and "uint64_t seed" in decl and "int32_t* draws" in decl
    schema = SCHEMA.replace("mi355ppo::", "")
    assert f'm.def("{schema}");' in cpp and 'm.impl("tactile_augment_seeded", tactile_augment_seeded);' in cpp
    kern = open(os.path.join(CSRC, "tactile_augment_seeded.h")).read()
    assert "void k_tactile_augment_seeded(" in kern and "IGI_E_UNSUPPORTED" in kern
    assert f"TAC_MAX_PIXELS = {ops.TACTILE_AUG_MAX_PIXELS};" in open(os.path.join(CSRC, "tactile_augment.h")).read()


@pytest.mark.parametrize("change, message", [
    (dict(arena=torch.zeros(6, 2, 3, 1, 9, 13, dtype=torch.float64)), "arena: expected dtype"),
    (dict(rows=torch.zeros(3, dtype=torch.int32)), "rows: expected dtype"),
    (dict(arena=torch.zeros(6, 6, 1, 9, 13)), "arena: expected 6 dimensions"),
    (dict(arena=torch.zeros(6, 6 * 9 * 13)), "arena: expected 6 dimensions"),
    (dict(rows=torch.zeros(3, 1, dtype=torch.int64)), "rows: expected 1 dimensions"),
    (dict(arena=torch.zeros(6, 2, 3, 1, 13, 9).transpose(4, 5)), "arena: expected a contiguous"),
    (dict(rows=torch.zeros(6, dtype=torch.int64)[::2]), "rows: expected a contiguous"),
    (dict(arena=torch.zeros(6, 2, 3, 3, 9, 13)), r"arena: expected \(R, T, F, 1, Hs, Ws\)"),
    (dict(arena=torch.zeros(0, 2, 3, 1, 9, 13)), r"arena: expected \(R, T, F, 1, Hs, Ws\) non-empty"),
    (dict(out_h=10), "out_h: expected 1..9"),
    (dict(out_h=0), "out_h: expected 1..9"),
    (dict(out_w=14), "out_w: expected 1..13"),
    (dict(patch=0), "patch: expected >= 1"),
    (dict(masking_prob=1.5), r"masking_prob: expected a value in \[0, 1\]"),
    (dict(masking_prob=-0.1), r"masking_prob: expected a value in \[0, 1\]"),
    (dict(masking_prob=float("nan")), r"masking_prob: expected a value in \[0, 1\]"),
    (dict(noise_std=-0.001), "noise_std: expected >= 0"),
    (dict(noise_std=float("nan")), "noise_std: expected >= 0"),
    (dict(), "expected a HIP"),                                   # everything else right, host tensors: no CPU path
])
def test_op_refuses_bad_arguments(change, message):
    args = {**_op_args(), **change}
    with pytest.raises(RuntimeError, match=message):
        torch.ops.mi355ppo.tactile_augment_seeded(*args.values())


def test_patch_zero_without_masking_is_not_looked_at():
    with pytest.raises(RuntimeError, match="expected a HIP"):     # past every argument check: refused for the device alone
        torch.ops.mi355ppo.tactile_augment_seeded(*{**_op_args(), "masking_prob": 0.0, "patch": 0}.values())
