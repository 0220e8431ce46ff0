"""k_pcl_augment (csrc/pcl_augment.h) against the float64 restatement tests/pcl_augment_ref.py, the golden cases taken
from the reference's ``PointCloudAugmentations`` (tests/golden/make_golden_pcl_augment.py) through the op, and
``ExtrinsicAdapt`` with ``task.env.pcl_augment: "fused"``.

Events -- hit, noise mask, contour and side flags, replaced index, axis, exempt, drop -- are integer comparisons of the same
hash on both sides, so they agree exactly: missed envs and dropped points are compared with ``torch.equal``, and a wrong
flag, index or axis would move a coordinate by far more than any bound below.  Values (``R.tolerance``), per coordinate:

  N  noise     2e-5 (sigma + const_noise) + 2^-22 (|x| + 2 noise_clip).  The kernel's z is within 2e-5 of the float64
               Box-Muller sample (the project's figure, tests/test_gpu_img_augment.py: logf / sqrtf / cosf of fp32 arguments);
               sigma z and const_noise pn scale it; the clamps are exact.  Three fp32 roundings remain -- sigma z (at most
               noise_clip after the clamp), x + j and + offset, each at most 2^-24 of a value below |x| + 2 noise_clip.
  R  rotation  2^-20 (|a| + |b|) + 1.5 N for a' = a cos + b sin.  cosf / sinf of the fp32 angle, |theta| <= pi, are
               within 2^-21 of the float64 values of the float64 angle, the angle's own three roundings ((2u - 1) rot_deg,
               the degree-to-radian constant and product) included: 2^-21 (|a| + |b|).  Two products and one sum round
               once each at 2^-24 of at most |a| + |b|: 3 x 2^-24 < 2^-21 - 2^-24.  The inputs carry N each, weighted by
               |cos| + |sin| <= sqrt 2 < 1.5.  The coordinate on the axis passes: N.
  O  outliers  max R over the cloud + 2e-5 max(1, outlier_scale) + 2^-22 |value|.  A contour outlier is hi + |z| or
               lo - |z|: hi / lo are coordinates of the cloud (min / max pick one, whatever the order), each within the
               largest R of the cloud; |z| within 2e-5; one rounding of the sum.  A free outlier is outlier_scale z: 2e-5
               outlier_scale and one rounding.
Missed envs, dropped points and everything with ``hit_prob = 0`` are exact."""
import os

import numpy as np
import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from tests import pcl_augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "pcl_augment.npz"))

# envs x objects: one point, under / at / over one pass of the 256 threads, two and three objects, the largest cloud
SHAPES = [(1, [1]), (3, [37]), (67, [256]), (3, [257]), (67, [400, 400]), (3, [5, 37, 300]), (3, [4096])]
STAGES = {"noise": dict(), "rotation": dict(rot_deg=30.0), "outliers": dict(outlier_ratio=0.1),
          "dropout": dict(dropout_ratio=0.2, no_dropout_prob=0.3),
          "all": dict(rot_deg=30.0, outlier_ratio=0.1, dropout_ratio=0.2, no_dropout_prob=0.3)}
SEED_EPISODE, SEED_STEP = 0x1234567887654321, 0x0FEDCBA987654321


def _cloud(N, points, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 1, sum(points) * 3, generator=g) * 0.25


def _episode(N):
    return (torch.arange(N, dtype=torch.int32) * 7) % 5


def _run(x, points, ep, q, se=SEED_EPISODE, ss=SEED_STEP):
    y = torch.ops.mi355ppo.pcl_augment(x.to(DEV), points, ep.to(DEV), q, se, ss)
    torch.cuda.synchronize()
    return y.cpu()


_REF = {}


def _ref(N, points, stage, hit_prob):
    key = (N, tuple(points), stage, hit_prob)
    if key not in _REF:
        x, ep, q = _cloud(N, points), _episode(N), R.params(hit_prob=hit_prob, **STAGES[stage])
        _REF[key] = (x, ep, q) + R.augment(x, points, ep, q, SEED_EPISODE, SEED_STEP)
    return _REF[key]


def _compare(y, x, points, q, ev, out):
    N, Pt = x.shape[0], sum(points)
    ratio = R.check(y, x, points, q, ev, out)
    print(f"N={N} points={points}: max |err| / bound = {ratio:.3f}, max |err| = {float((y.double() - out).abs().max()):.3e}")
    assert ratio <= 1.0
    hit = torch.from_numpy(ev["hit"])
    assert torch.equal(y[~hit], x[~hit])                                             # missed envs: bit for bit
    assert torch.equal((y.reshape(N, Pt, 3) == 0).all(-1), torch.from_numpy(ev["drop"]))
    far = ((y.double() - torch.from_numpy(ev["after_rot"]).reshape(x.shape)).abs() > 1e-4).reshape(N, Pt, 3).any(-1)
    assert torch.equal(far | torch.from_numpy(ev["drop"]), torch.from_numpy(ev["replaced"] | ev["drop"]))


@pytest.mark.parametrize("N, points", SHAPES, ids=lambda v: str(v))
def test_everything_off_or_missed_is_the_input(N, points):
    x, ep = _cloud(N, points), _episode(N)
    y = _run(x, points, ep, R.params(hit_prob=0.0, **STAGES["all"]))
    assert torch.equal(y, x)
    y = _run(x, points, ep, R.params(hit_prob=0.0))
    assert torch.equal(y, x)
    y = _run(x, points, ep, R.params(hit_prob=1.0, sigma=0.0, const_noise=0.0))      # every stage at "nothing"
    assert torch.equal(y, x)


@pytest.mark.parametrize("N, points", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("stage", ["noise", "rotation", "outliers", "dropout"])
def test_each_stage_alone(stage, N, points):
    x, ep, q, out, ev = _ref(N, points, stage, 1.0)
    y = _run(x, points, ep, q)
    _compare(y, x, points, q, ev, out)
    y3 = _run(x.reshape(N, -1, 3), points, ep, q)                                    # the (N, P_total, 3) layout
    assert y3.shape == (N, sum(points), 3) and torch.equal(y3.reshape(x.shape), y)


@pytest.mark.parametrize("N, points", SHAPES, ids=lambda v: str(v))
def test_whole_chain(N, points):
    x, ep, q, out, ev = _ref(N, points, "all", 0.7)
    y = _run(x, points, ep, q)
    _compare(y, x, points, q, ev, out)
    if N >= 67:
        assert ev["hit"].any() and not ev["hit"].all() and ev["drop"].any() and ev["replaced"].any()
        assert set(ev["axis"][ev["hit"]].tolist()) == {0, 1, 2}


def test_four_objects():
    points, N = [37, 5, 300, 64], 5
    x, ep, q = _cloud(N, points), _episode(N), R.params(hit_prob=0.8, **STAGES["all"])
    out, ev = R.augment(x, points, ep, q, SEED_EPISODE, SEED_STEP)
    _compare(_run(x, points, ep, q), x, points, q, ev, out)


def test_4097_points_are_refused_and_fused_falls_back():
    from isaacgyminsertion_amd.envs.pcl_augment import PclAugment
    points, N = [4097], 2
    x, ep = _cloud(N, points).to(DEV), _episode(N).to(DEV)
    with pytest.raises(RuntimeError, match=r"points\[0\]: expected 1..4096"):
        torch.ops.mi355ppo.pcl_augment(x, points, ep, R.params(), 1, 2)
    a = PclAugment(points, hit_prob=1.0, outlier_ratio=0.01, seed=9)
    y = a.fused(x, ep)
    assert y.device == x.device and y.shape == x.shape and a.seed_step is not None
    assert torch.equal(y, a.apply(x, ep, a.seed_step))
    out, ev = R.augment(x.cpu(), points, ep.cpu(), a.params(), a.seed_episode, a.seed_step)
    assert R.check(y.cpu(), x.cpu(), points, a.params(), ev, out) <= 1.0 and ev["replaced"].sum() > 0


def test_no_outliers_at_five_points():
    points, N = [5], 9
    x, ep = _cloud(N, points), _episode(N)
    assert int(5 * 0.1) == 0
    y = _run(x, points, ep, R.params(hit_prob=1.0, outlier_ratio=0.1))
    assert torch.equal(y, _run(x, points, ep, R.params(hit_prob=1.0)))
    out, ev = R.augment(x, points, ep, R.params(hit_prob=1.0, outlier_ratio=0.1), SEED_EPISODE, SEED_STEP)
    assert not ev["replaced"].any()
    _compare(y, x, points, R.params(hit_prob=1.0, outlier_ratio=0.1), ev, out)


def test_duplicate_indices_the_highest_k_wins():
    points, N, seed = [40], 4, 5550001                                  # cloud 1 draws the indices 22, 19, 27, 19
    x, ep = _cloud(N, points), torch.zeros(N, dtype=torch.int32)
    q = R.params(hit_prob=1.0, outlier_ratio=0.1, sigma=0.0, const_noise=0.0)
    out, ev = R.augment(x, points, ep, q, SEED_EPISODE, seed)
    assert ev["index"][1, :4].tolist() == [22, 19, 27, 19] and ev["winner"][1, 19] == 3
    _compare(_run(x, points, ep, q, ss=seed), x, points, q, ev, out)


@pytest.mark.parametrize("tag", ["noise", "dropout", "outliers"])
def test_golden_cases_through_the_op(tag):
    x64 = torch.from_numpy(G[f"{tag}/x"])
    x = x64.float()
    assert torch.equal(x.double(), x64)                                 # the fixture holds fp32 values
    kw = {"noise": dict(), "dropout": dict(sigma=0.0, const_noise=0.0, dropout_ratio=float(G["dropout/ratio"]),
                                          no_dropout_prob=float(G["dropout/no_dropout_prob"])),
          "outliers": dict(sigma=0.0, const_noise=0.0, outlier_ratio=0.1)}[tag]
    q, points, ep = R.params(hit_prob=1.0, **kw), [x.shape[1]], torch.zeros(4, dtype=torch.int32)
    se, ss, gold = int(G["noise/seed_episode"]), int(G[f"{tag}/seed"]), torch.from_numpy(G[f"{tag}/y"])
    y = _run(x, points, ep, q, se, ss)
    _out, ev = R.augment(x, points, ep, q, se, ss)
    if tag == "dropout":
        assert torch.equal(y.double(), gold)
    else:
        ratio = R.check(y, x, points, q, ev, gold)                      # against the REFERENCE's result
        print(f"{tag}: max |err| / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_repeats_seeds_and_the_input():
    N, points = 67, [400, 400]
    x, ep, q = _cloud(N, points).to(DEV), _episode(N).to(DEV), R.params(hit_prob=0.7, **STAGES["all"])
    keep, keep_ep = x.clone(), ep.clone()
    op = torch.ops.mi355ppo.pcl_augment
    y1, y2 = op(x, points, ep, q, SEED_EPISODE, SEED_STEP), op(x, points, ep, q, SEED_EPISODE, SEED_STEP)
    assert torch.equal(y1, y2) and y1.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep) and torch.equal(ep, keep_ep)           # neither input is written
    assert not torch.equal(op(x, points, ep, q, SEED_EPISODE, SEED_STEP + 1), y1)
    assert not torch.equal(op(x, points, ep, q, SEED_EPISODE + 1, SEED_STEP), y1)
    assert not torch.equal(op(x, points, ep + 1, q, SEED_EPISODE, SEED_STEP), y1)
    # the per-episode draws follow the counter of their own env only
    ep2 = ep.clone()
    ep2[5] += 1
    y3 = op(x, points, ep2, q, SEED_EPISODE, SEED_STEP)
    rows = torch.arange(N, device=DEV) != 5
    assert torch.equal(y3[rows], y1[rows])


def test_opcheck():
    N, points = 3, [5, 37]
    args = (_cloud(N, points).to(DEV), points, _episode(N).to(DEV))
    tests = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_static")
    torch.library.opcheck(torch.ops.mi355ppo.pcl_augment, args + (R.params(), 1, 2), test_utils=tests)
    torch.library.opcheck(torch.ops.mi355ppo.pcl_augment, args + (R.params(**STAGES["all"]), 3, 4), test_utils=tests)


# ---- the trainer ----------------------------------------------------------------------------------------------------------
N_ENVS, HORIZON, PTS = 64, 4, [37, 37]


def _agent(key, seed=0):
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=N_ENVS, horizon_length=HORIZON, rl_device=DEV, mini_epochs=2, obs_info=True, pcl_info=True)
    cfg.task.env.num_points, cfg.task.env.num_points_socket = PTS
    if key is None:
        cfg.task.env.pop("pcl_augment")
    else:
        cfg.task.env.pcl_augment = key
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    env = SyntheticInsertionEnv(N_ENVS, device=DEV, pcl_points=sum(PTS), done_p=0.2)
    agent = ExtrinsicAdapt(env, None, cfg)
    agent.obs = env.reset()
    return agent, env


def _rollout(agent, env):
    """One ``play_steps`` under the profiler, from reseeded global generators -> (kernel / op names, the global generators'
    states afterwards, the env's dones per step)."""
    from torch.profiler import ProfilerActivity, profile
    dones, step = [], env.step

    def spy(actions):
        r = step(actions)
        dones.append(r[2].clone())
        return r
    env.step = spy
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    agent.set_student_eval()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        agent.play_steps()
        torch.cuda.synchronize()
    env.step = step
    return [e.name for e in prof.events()], (torch.get_rng_state(), torch.cuda.get_rng_state(DEV)), dones


def test_trainer_with_the_key_on():
    from isaacgyminsertion_amd.algo.models.running_mean_std import RunningMeanStd
    agent, env = _agent("fused")
    aug = agent.pcl_augment
    assert aug is not None and aug.points == PTS and aug.params() == R.params(hit_prob=0.7)
    calls, fused = [], aug.fused

    def spy(clouds, episode):
        y = fused(clouds, episode)
        calls.append((clouds.clone(), episode.clone(), aug.seed_step, y.clone()))
        return y
    aug.fused = spy
    names, rng_on, dones = _rollout(agent, env)
    assert len(calls) == HORIZON and len(dones) == HORIZON
    # one launch per rollout step, no boolean-mask indexing anywhere in the rollout
    assert sum("k_pcl_augment" in n for n in names) == HORIZON
    assert sum(n == "mi355ppo::pcl_augment" for n in names) == HORIZON
    assert not any(n == "aten::nonzero" for n in names)
    # the op's outputs are the restatement's for the recorded seeds and counters; n_pcl is their normalisation
    rms = RunningMeanStd((3,)).to(DEV)
    rms.train()
    total = torch.zeros(N_ENVS, dtype=torch.int32)
    for n, (clouds, episode, seed_step, y) in enumerate(calls):
        assert torch.equal(episode.cpu(), total)                      # the counters the step saw: the dones before it
        out, ev = R.augment(clouds.cpu(), PTS, episode.cpu(), aug.params(), aug.seed_episode, seed_step)
        assert R.check(y.cpu(), clouds.cpu(), PTS, aug.params(), ev, out) <= 1.0
        assert ev["hit"].any() and not ev["hit"].all()
        want = rms(y.reshape(-1, 3)).reshape(N_ENVS, 1, -1)
        assert torch.equal(agent.storage.storage_dict["n_pcl"][n], want.reshape(agent.storage.storage_dict["n_pcl"][n].shape))
        total += dones[n].cpu().reshape(-1).to(torch.int32)
    assert torch.equal(agent.pcl_episode.cpu(), total) and int(total.sum()) > 0
    # torch's global generators: as in a run without the key
    plain, env2 = _agent(None)
    _names, rng_off, _d = _rollout(plain, env2)
    assert torch.equal(rng_on[0], rng_off[0]) and torch.equal(rng_on[1], rng_off[1])
    aug.fused = fused
    action_losses, _latent = agent.train_epoch()
    assert len(action_losses) > 0 and all(bool(torch.isfinite(l).all()) for l in action_losses)


def test_trainer_with_the_key_off_is_the_trainer_without_it():
    results = []
    for key in (None, "off"):
        agent, env = _agent(key)
        assert agent.pcl_augment is None and agent.pcl_episode is None
        names, _rng, _d = _rollout(agent, env)
        assert not any("k_pcl_augment" in n for n in names)
        agent.set_student_train()
        loss, _ = agent.update_step(0)
        results.append((agent.storage.storage_dict["n_pcl"].clone(), loss.detach().clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
