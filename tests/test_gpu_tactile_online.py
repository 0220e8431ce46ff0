"""k_tactile_augment_seeded (csrc/tactile_augment_seeded.h) through torch.ops.mi355ppo.tactile_augment_seeded,
TactileAugment.fused_seeded and ExtrinsicAdapt's distillation step, against the float64 restatement
tests/tactile_online_ref.py (layered on tests/tactile_augment_ref.py).

Arenas of T*N = 6 flat rows; planes 1 x 3 and 2 x 3; images 32 x 64, 9 x 13 (patch 4: a partial last patch) and 64 x 64;
batches of 5 rows with one repeated row and one row outside the arena; one case of 67 images.  Seeds: ``O.SEEDS``, chosen on
the CPU (tests/test_tactile_online_cpu.py asserts the tie share of every one of them).

The draws are exact: ``draws`` is ``torch.equal`` to the restatement's.  The image chain is held to the bounds of
tests/test_gpu_tactile_augment.py, unchanged: gather and patch masking exact; the rotation exact on every pixel whose float64
source coordinate is farther than 1e-4 from a rounding tie; the jitter within ``R.jitter_bound(pixels)``; and with d = output
- noise-free output of the same call, |d - noise_std * z_ref| <= 2e-5 * noise_std + 2^-22 * (|pixel| + 6 * noise_std)."""
import numpy as np
import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import tactile_augment_ref as R
from tests import tactile_online_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = torch.tensor(O.ROWS)
CASE_IDS = [f"{T}x{Fg}-{H}x{W}-p{p}" for T, Fg, H, W, p in O.CASES]


def _op(arena, rows, patch, noise_std=0.0, masking_prob=0.0, seed=0, want_draws=False):
    y, d = torch.ops.mi355ppo.tactile_augment_seeded(arena.to(DEV), rows.to(DEV), arena.shape[-2], arena.shape[-1], patch,
                                                     noise_std, masking_prob, seed, want_draws)
    return y.cpu(), (None if d is None else d.cpu())


@pytest.fixture(scope="module")
def clean():
    """Every case x seed without noise or masking, computed once: (arena, op output, restatement, band, draws)."""
    out = {}
    for k, (T, Fg, H, W, patch) in enumerate(O.CASES):
        arena = O.arena(T, Fg, H, W, seed=k)
        for seed in O.SEEDS:
            y, d = _op(arena, ROWS, patch, seed=seed, want_draws=True)
            ref, band, draws = O.augment(arena, ROWS, seed, patch)
            out[(k, seed)] = (arena, y, d, ref, band, draws)
    return out


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_draws_are_the_restatements_bit_for_bit(clean, k):
    T, Fg, H, W, patch = O.CASES[k]
    for seed in O.SEEDS:
        arena, y, d, _ref, _band, (off, jit, ang, _keep) = clean[(k, seed)]
        assert y.shape == (5, T, Fg, 1, H, W) and d.shape == (5 * T * Fg, 6) and d.dtype == torch.int32
        assert torch.equal(d, O.packed(off, jit, ang))                                # flags, factor bits, angle bits
        assert d[:, 2].any() and not d[:, 2].all() and (d[:, 5] != 0).any() and not (d[:, 5] != 0).all()
        # the draws do not depend on whether they are asked for, nor on noise or masking
        y2, none = _op(arena, ROWS, patch, seed=seed)
        assert none is None and torch.equal(y2, y)
        _y, d3 = _op(arena, ROWS, patch, 0.01, 0.3, seed, True)
        assert torch.equal(d3, d)


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_images_with_both_flags_off_are_the_gathered_input(clean, k):
    T, Fg, H, W, _patch = O.CASES[k]
    seen = 0
    for seed in O.SEEDS:
        arena, y, _d, _ref, _band, (_off, jit, ang, _keep) = clean[(k, seed)]
        still = ((jit[:, 0] == 0) & (ang == 0)).reshape(5, T, Fg)
        gathered = torch.cat([arena.index_select(0, ROWS[:4]), torch.zeros(1, *arena.shape[1:])])
        assert torch.equal(y[still], gathered[still]) and (gathered[still] < 0).any()     # no clamp: negatives pass
        assert not y[4].any()                                                         # the row outside the arena: zeros
        seen += int(still[:4].sum())
    assert seen >= 3


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_jitter_and_rotation_are_within_the_unchanged_bounds(clean, k):
    T, Fg, H, W, _patch = O.CASES[k]
    bound = R.jitter_bound(H * W)
    n = 5 * T * Fg
    both = 0
    for seed in O.SEEDS:
        arena, y, _d, ref, band, (off, jit, ang, _keep) = clean[(k, seed)]
        y, ref, band = y.reshape(n, H, W).double(), ref.reshape(n, H, W), band.reshape(n, H, W)
        share = float(band.double().mean())
        assert share <= O.TIE_SHARE_MAX
        on = jit[:, 0] != 0
        assert torch.equal(torch.where(band, ref, y)[~on], ref[~on])                     # no jitter: equal off the tie band
        err = torch.where(band, torch.zeros_like(ref), (y - ref).abs())[on].amax(dim=(1, 2))
        print(f"{CASE_IDS[k]} seed {seed}: jitter max err {err.max():.3e}, bound {bound:.3e}, excluded share {share:.5f}")
        assert (err <= bound).all()
        assert (y[on] >= 0).all() and (y[on] <= 1).all()
        # jitter happens BEFORE the rotation: the other order -- zero-fill the rim, then take the mean -- is far outside
        live = torch.tensor(O.ROWS).repeat_interleave(T * Fg) < O.ARENA_ROWS
        turned = on & live & (ang.abs() > 0.02)
        if (H, W) != (9, 13) and turned.any():        # (at 9 x 13 three degrees move no pixel: the rotation is a copy)
            w = R.window(arena, ROWS, off, H, W)
            rev = R.jitter_images(torch.where((ang != 0)[:, None, None, None], R.rotate(w, ang), w), jit).reshape(n, H, W)
            far = torch.where(band, torch.zeros_like(ref), (y - rev).abs()).amax(dim=(1, 2))
            assert (far[turned] > 1e2 * bound).all()
            both += int(turned.sum())
    assert both >= 1 or (H, W) == (9, 13)


@pytest.mark.parametrize("k", range(len(O.CASES)), ids=CASE_IDS)
def test_masked_cells_are_zero_and_kept_cells_untouched(clean, k):
    T, Fg, H, W, patch = O.CASES[k]
    seed = O.SEEDS[k % len(O.SEEDS)]
    arena, y, _d, _ref, _band, _draws = clean[(k, seed)]
    ym, _ = _op(arena, ROWS, patch, 0.0, 0.3, seed)
    keep = O.draws(5 * T * Fg, seed, H, W, patch, 0.3)[3]
    mask = R.patch_mask(keep, H, W, patch).reshape(y.shape)
    assert 0 < keep.sum() < keep.numel() and len({tuple(g.flatten().tolist()) for g in keep}) > keep.shape[0] // 2
    assert torch.equal(ym.double(), y.double() * mask)             # exact zeros, and the kept cells bit for bit
    gh, gw = H // patch, W // patch
    dropped = mask == 0
    assert not dropped[..., gh * patch:, :].any() and not dropped[..., :, gw * patch:].any()   # the partial last patch is kept
    # after noise the mask still zeroes the OUTPUT cells
    yn, _ = _op(arena + 1.5, ROWS, patch, 0.05, 0.3, seed)
    assert (yn[dropped] == 0).all() and (yn[:4][~dropped[:4]] != 0).float().mean() > 0.9
    # masking_prob 1 keeps nothing but the rim past the last whole patch; 0 is no mask at all
    y1, _ = _op(arena + 1.5, ROWS, patch, 0.0, 1.0, seed)
    assert not y1[..., :gh * patch, :gw * patch].any()
    if (H, W) == (9, 13):
        assert y1[:4][..., 8:, :].all() and y1[:4][..., :, 12:].all()


@pytest.mark.parametrize("k, std", [(0, 0.001), (1, 0.05), (3, 0.05)], ids=["1x3-32x64", "2x3-32x64", "2x3-9x13"])
def test_noise_is_the_hashed_gaussian_of_plane_two(clean, k, std):
    T, Fg, H, W, patch = O.CASES[k]
    seed = O.SEEDS[1]
    arena, base, _d, _ref, _band, _draws = clean[(k, seed)]
    noisy, _ = _op(arena, ROWS, patch, std, 0.0, seed)
    z_ref = R.gauss(seed, R.NOISE_PLANE, base.shape)
    s = float(np.float32(std))
    d = noisy.double() - base.double()
    err = (d - s * z_ref).abs()
    bound = 2e-5 * s + 2.0 ** -22 * (base.double().abs() + 6 * s)
    print(f"{CASE_IDS[k]} std {std}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    for plane in (0, 1):                                           # not the camera pair's planes
        assert (d - s * R.gauss(seed, plane, base.shape)).abs().max() > std
    other, _ = _op(arena, ROWS, patch, std, 0.0, seed + 1)
    assert not torch.allclose(other, noisy, atol=0.1 * std)


def test_sixty_seven_images():
    B, T, Fg, H, W, patch = O.MANY
    arena = O.arena(T, Fg, H, W, seed=9)
    rows = (torch.arange(B) * 5) % (O.ARENA_ROWS + 1)              # every row, the one outside the arena included
    for seed in O.SEEDS[:2]:
        y, d = _op(arena, rows, patch, 0.0, 0.3, seed, True)
        ref, band, (off, jit, ang, keep) = O.augment(arena, rows, seed, patch, 0.0, 0.3)
        assert torch.equal(d, O.packed(off, jit, ang)) and band.double().mean() <= O.TIE_SHARE_MAX
        err = torch.where(band, torch.zeros_like(ref), (y.double() - ref).abs())
        assert err.max() <= R.jitter_bound(H * W)
        on = (jit[:, 0] != 0).reshape(B, 1, 1)
        assert torch.equal(torch.where(band, ref, y.double())[~on], ref[~on])
        assert not y[rows == O.ARENA_ROWS].any() and (rows == O.ARENA_ROWS).sum() >= 5


def test_repeats_are_bit_identical_and_the_input_is_untouched():
    T, Fg, H, W, patch = O.CASES[1]
    arena = O.arena(T, Fg, H, W, seed=4).to(DEV)
    before = arena.clone()
    rows = ROWS.to(DEV)
    call = lambda seed: torch.ops.mi355ppo.tactile_augment_seeded(arena, rows, H, W, patch, 0.01, 0.3, seed, True)  # noqa: E731
    (y1, d1), (y2, d2), (y3, d3) = call(O.SEEDS[0]), call(O.SEEDS[0]), call(O.SEEDS[1])
    assert torch.equal(y1, y2) and torch.equal(d1, d2) and torch.equal(arena, before)
    assert not torch.equal(y1, y3) and not torch.equal(d1, d3)
    # rows in another order: image i's draws go with its place in the batch, its pixels with its row
    _y, d4 = torch.ops.mi355ppo.tactile_augment_seeded(arena, rows.flip(0), H, W, patch, 0.01, 0.3, O.SEEDS[0], True)
    assert torch.equal(d4, d1)
    # an output that is no multiple of 16 bytes from its base takes the scalar stores: same bits
    y0, _ = torch.ops.mi355ppo.tactile_augment_seeded(arena, rows[:0], H, W, patch, 0.01, 0.3, 1, False)
    assert y0.shape == (0, T, Fg, 1, H, W)


def test_a_window_larger_than_the_kernels_is_refused_and_fused_seeded_takes_the_torch_path():
    from isaacgyminsertion_amd.algo.models.transformer.utils import TactileAugment
    big = torch.rand(2, 1, 1, 1, 96, 96, generator=torch.Generator().manual_seed(0)).to(DEV)
    rows = torch.tensor([1, 0], device=DEV)
    with pytest.raises(RuntimeError, match="igi_tactile_augment_seeded"):
        torch.ops.mi355ppo.tactile_augment_seeded(big, rows, 96, 96, 8, 0.0, 0.0, 1, False)
    aug = TactileAugment((96, 96), (96, 96), 8, 0.01, 0.3)
    y, d = aug.fused_seeded(big.reshape(2, -1), rows, O.SEEDS[0], want_draws=True, fingers=1)
    off, jit, ang, keep, s = aug.draw_seeded(2, O.SEEDS[0])
    assert y.shape == (2, 1, 1, 1, 96, 96) and torch.isfinite(y).all()
    assert torch.equal(d.cpu(), aug.pack(off, jit, ang))
    assert torch.equal(y, aug.apply(big.index_select(0, rows), off, jit, ang, keep, 0.01, s))
    # 8192 pixels is the largest window the kernel takes
    edge = torch.rand(1, 1, 1, 1, 64, 128, generator=torch.Generator().manual_seed(1))
    seed = O.EDGE_SEED                                             # image 0 is jittered and turned under it
    y, _ = _op(edge, torch.zeros(1, dtype=torch.int64), 16, seed=seed)
    ref, band, _draws = O.augment(edge, torch.zeros(1, dtype=torch.int64), seed, 16)
    assert torch.where(band, torch.zeros_like(ref), (y.double() - ref).abs()).max() <= R.jitter_bound(8192)
    # fused_seeded on the kernel's path is the op on the arena as the gather sees it
    T, Fg, H, W, patch = O.CASES[1]
    arena = O.arena(T, Fg, H, W, seed=4).to(DEV)
    aug = TactileAugment((H, W), (H, W), patch, 0.01, 0.3)
    y, d = aug.fused_seeded(arena.reshape(O.ARENA_ROWS, -1), ROWS.to(DEV), O.SEEDS[2], want_draws=True)
    y2, d2 = torch.ops.mi355ppo.tactile_augment_seeded(arena, ROWS.to(DEV), H, W, patch, 0.01, 0.3, O.SEEDS[2], True)
    assert y.shape == (5, T, Fg, 1, H, W) and torch.equal(y, y2) and torch.equal(d, d2)


def test_opcheck():
    T, Fg, H, W, patch = O.CASES[3]
    arena = O.arena(T, Fg, H, W, seed=7).to(DEV)
    tests = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
    op = torch.ops.mi355ppo.tactile_augment_seeded
    torch.library.opcheck(op, (arena, ROWS.to(DEV), H, W, patch, 0.01, 0.3, 11, True), test_utils=tests)
    torch.library.opcheck(op, (arena, ROWS.to(DEV), H, W, 1, 0.0, 0.0, 0, False), test_utils=tests)


# ---- the trainer ----------------------------------------------------------------------------------------------------------
E = O.ENGINE
STEPS = E["mini_epochs"] * E["mini_epochs"]                          # optimizer steps per epoch: 4 minibatches x 4 mini-epochs
MB = E["envs"] * E["horizon"] // E["mini_epochs"]


def _agent(key, seed=0):
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=E["envs"], horizon_length=E["horizon"], rl_device=DEV, mini_epochs=E["mini_epochs"],
                         obs_info=True, tactile_info=True, pcl_info=False, img_info=False, seg_info=False, num_points=8)
    assert cfg.seed == E["seed"]
    if key is None:
        cfg.offline_train.pop("tactile_augment_online")
    else:
        cfg.offline_train.tactile_augment_online = key
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    env = SyntheticInsertionEnv(E["envs"], device=DEV, tactile_hw=(32, 64), pcl_points=0, img_hw=None)
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


def test_trainer_with_the_key_on(monkeypatch):
    from isaacgyminsertion_amd.algo.ppo import experience
    agent, _env = _agent("fused")
    aug = agent.tactile_augment
    assert aug is not None and (aug.patch, aug.noise_std, aug.masking_prob) == (16, 0.001, 0.0)
    names, _kernels = _rollout(agent)
    assert not any("k_tactile_augment_seeded" in n or "tactile_augment_seeded" in n for n in names)   # the rollout: none of it
    assert agent.tactile_seed is None
    arena = agent.storage.storage_dict["n_tactile"]
    stored = arena.clone()
    calls, fused, prefetched, batches = [], aug.fused_seeded, [], []

    def spy(arena2d, rows, seed, want_draws=False, fingers=3):
        y, _ = fused(arena2d, rows, seed, want_draws, fingers)
        calls.append((arena2d.data_ptr(), tuple(arena2d.shape), rows.clone(), seed, y.detach().clone()))
        return y, None
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
    # one optimizer step under the profiler: one launch of the kernel, and the gather no longer moves the tactile rows
    agent.set_student_train()
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    names, kernels = _profiled(lambda: agent.update_step(0))
    rng_on = (torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
    assert sum("k_tactile_augment_seeded" in n for n in names) == 1
    assert sum(n == "mi355ppo::tactile_augment_seeded" for n in names) == 1
    assert sum(n == "mi355ppo::gather_rows" for n in names) == 1
    assert "n_tactile" not in prefetched[0] and "n_student_obs" in prefetched[0]
    assert "n_tactile" not in batches[0]._c and "n_student_obs" in batches[0]._c          # never gathered
    agent.optim.step(1.0)
    # torch's global generators: where the same step leaves them in a trainer without the key
    plain, _env2 = _agent(None)
    _rollout(plain)
    plain.set_student_train()
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    plain.update_step(0)
    assert torch.equal(torch.get_rng_state(), rng_on[0]) and torch.equal(torch.cuda.get_rng_state(DEV), rng_on[1])
    del plain
    # a whole epoch's update: one launch per optimizer step, every loss finite
    names, kernels = _profiled(agent.update)
    assert sum("k_tactile_augment_seeded" in n for n in names) == STEPS and len(calls) == 1 + STEPS
    # the step's tactile input is the restatement's for the recorded seeds
    assert [c[3] for c in calls] == O.engine_seeds(1 + STEPS) and agent.tactile_seed == calls[-1][3]
    assert torch.equal(arena, stored)                                                     # the arena is read in place
    cpu_arena = stored.reshape(E["envs"] * E["horizon"], 1, 3, 1, 32, 64).cpu()
    bound = R.jitter_bound(2048)
    for ptr, shape, rows, seed, y in calls[:6]:
        assert ptr == arena.data_ptr() and shape == (E["envs"] * E["horizon"], 3 * 2048) and rows.numel() == MB
        y = y.cpu()
        assert y.shape == (MB, 1, 3, 1, 32, 64)
        base, _ = _op(cpu_arena, rows.cpu(), 16, 0.0, 0.0, seed)
        ref, band, (_off, jit, _ang, _keep) = O.augment(cpu_arena, rows.cpu(), seed, 16)
        assert band.double().mean() <= O.TIE_SHARE_MAX
        err = torch.where(band, torch.zeros_like(ref), (base.double() - ref).abs())
        assert err.max() <= bound
        on = (jit[:, 0] != 0).reshape(MB, 1, 3)
        assert torch.equal(torch.where(band, ref, base.double())[~on], ref[~on])
        s = float(np.float32(0.001))
        d = y.double() - base.double()
        noise_err = (d - s * R.gauss(seed, R.NOISE_PLANE, y.shape)).abs()
        assert (noise_err <= 2e-5 * s + 2.0 ** -22 * (base.double().abs() + 6 * s)).all()
    aug.fused_seeded = fused
    monkeypatch.undo()
    # one whole train_epoch: rollout (unaugmented) + update
    agent.obs = _env.reset()
    action_losses, _latent = agent.train_epoch()
    assert len(action_losses) == STEPS and all(bool(torch.isfinite(l).all()) for l in action_losses)


def test_trainer_with_the_key_off_is_the_trainer_without_it():
    results = []
    for key in (None, "off"):
        agent, _env = _agent(key)
        assert agent.tactile_augment is None and agent.tactile_seed is None
        _rollout(agent)
        agent.set_student_train()
        loss, _ = agent.update_step(0)
        agent.optim.step(1.0)
        names, kernels = _profiled(lambda: agent.update_step(1))
        assert not any("tactile_augment_seeded" in n for n in names)
        results.append((loss.detach().clone(), kernels, agent.storage.storage_dict["n_tactile"].clone()))
    assert torch.equal(results[0][0], results[1][0]) and bool(torch.isfinite(results[0][0]).all())
    assert results[0][1] == results[1][1] and len(results[0][1]) > 10
    assert torch.equal(results[0][2], results[1][2])
