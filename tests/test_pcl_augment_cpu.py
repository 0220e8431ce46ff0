"""Point-cloud augmentation of the online student, host side: the float64 restatement the GPU tests compare against
(tests/pcl_augment_ref.py) on the golden cases taken from the reference's ``PointCloudAugmentations``
(tests/golden/make_golden_pcl_augment.py), ``PclAugment.draw`` / ``apply``, the ``task.env.pcl_augment`` key of
``ExtrinsicAdapt`` with its default-off rule, and the op's schema, fake kernel and refusals (they raise before any launch).
Bounds N / R / O: tests/pcl_augment_ref.py ``tolerance`` (derived in tests/test_gpu_pcl_augment.py).  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

from isaacgyminsertion_amd import ops  # noqa: F401  (registers torch.ops.mi355ppo)
from oracle.token_dropout import threshold, tok_hash
from tests import pcl_augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "pcl_augment.npz"))
ALL_ON = dict(hit_prob=0.8, rot_deg=30.0, outlier_ratio=0.1, dropout_ratio=0.2, no_dropout_prob=0.3)


def _P():
    from isaacgyminsertion_amd.envs import pcl_augment
    return pcl_augment


def _cloud(N, points, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, 1, sum(points) * 3, generator=g, dtype=torch.float32) * 0.25).to(dtype)


def _zeros(N):
    return torch.zeros(N, dtype=torch.int32)


def test_names_through_both_import_paths():
    P = _P()
    import algo.ext_adapt.ext_adapt as shim
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    assert shim.PclAugment is ext_adapt.PclAugment is P.PclAugment
    assert hasattr(P, "PointCloudAugmentations")
    a = P.PclAugment([400, 400])
    assert (a.hit_prob, a.rot_deg, a.outlier_ratio, a.dropout_ratio) == (0.7, 0.0, 0.0, 0.0)
    assert (a.sigma, a.noise_clip, a.const_noise, a.noise_prob) == (0.001, 0.001, 0.001, 0.3)
    assert (a.contour_prob, a.outlier_scale, a.no_dropout_prob) == (0.75, 1.5, 0.8)
    assert a.params() == R.params() and tuple(ops.PCL_AUG_PARAMS) == R.ORDER
    for bad in (dict(hit_prob=1.5), dict(sigma=-1.0), dict(outlier_ratio=-0.1), dict(rot_deg=-3.0)):
        with pytest.raises(ValueError):
            P.PclAugment([5], **bad)
    with pytest.raises(ValueError):
        P.PclAugment([])


def test_header_table_and_python_tables_agree():
    from isaacgyminsertion_amd import draws
    hdr = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "draws.h")).read()
    for name in ("PN", "JITTER", "FREE", "CONTOUR"):
        v = int(re.search(rf"PCL_PLANE_{name} = (\d+)", hdr).group(1))
        assert v == draws.PLANES[f"PCL_PLANE_{name}"] == getattr(R, f"PLANE_{name}") and v > 2      # planes 0..2 are taken
    for name in ("HIT", "ANGLE", "AXIS", "MASK", "CONTOUR", "SIDE", "INDEX", "EXEMPT", "DROP"):
        v = int(re.search(rf"PCL_SITE_{name} = (\d+)", hdr).group(1))
        assert v == draws.SITES[f"PCL_SITE_{name}"] == getattr(R, f"SITE_{name}") and v > 13        # sites 0..13 are the planes'
    idx = np.arange(1000)
    for seed in (0, 12345678901234567, 2 ** 64 - 1):
        assert np.array_equal(draws.tok_hash(seed, 17, torch.from_numpy(idx)).numpy(), tok_hash(seed, 17, idx).astype(np.int64))
    for p in (0.0, 0.1, 0.3, 0.5, 0.75):
        assert draws.threshold(p) == int(threshold(p))
    assert draws.threshold(1.0) == 2 ** 32                          # above every hash: always


# ---- the restatement against the reference's arithmetic ------------------------------------------------------------------
def test_restatement_rotation_golden():
    x, y, deg, axes = G["rot/x"], G["rot/y"], G["rot/angles_deg"], G["rot/axes"]
    assert x.shape == (5, 7, 3) and set(axes.tolist()) == {0, 1, 2} and {0.0, 30.0, -30.0} <= set(deg.tolist())
    q = R.params(sigma=0.0, const_noise=0.0)
    tol = R.bound_rot(x, axes, q)
    for b in range(5):
        got = R.rotate(x[b], deg[b] * (math.pi / 180), int(axes[b]))
        assert (np.abs(got - y[b]) <= tol[b]).all()
    assert np.array_equal(R.rotate(x[0], 0.0, 0), x[0])


def test_restatement_offset_golden():
    x, pn, y = G["offset/x"], G["offset/pn"], G["offset/y"]
    assert (np.abs(pn) > 1).any() and (np.abs(pn) < 1).any()        # the clamp bites on some, not all
    off = R.const_offset(pn, 0.001, 0.001)
    assert np.abs(off).max() == R.f32(0.001) and (np.abs(off) < R.f32(0.001)).any()
    got = x + off[:, None, :]
    assert (np.abs(got - y) <= R.bound_noise(x, R.params(sigma=0.0))).all()


def _golden_case(tag):
    x = torch.from_numpy(G[f"{tag}/x"])
    kw = {"noise": dict(), "dropout": dict(sigma=0.0, const_noise=0.0, dropout_ratio=float(G["dropout/ratio"]),
                                          no_dropout_prob=float(G["dropout/no_dropout_prob"])),
          "outliers": dict(sigma=0.0, const_noise=0.0, outlier_ratio=0.1)}[tag]
    q = R.params(hit_prob=1.0, **kw)
    return x, [x.shape[1]], q, int(G["noise/seed_episode"]), int(G[f"{tag}/seed"]), torch.from_numpy(G[f"{tag}/y"])


@pytest.mark.parametrize("tag", ["noise", "dropout", "outliers"])
def test_restatement_reproduces_the_reference_on_our_draws(tag):
    x, points, q, se, ss, y = _golden_case(tag)
    assert x.shape[:2] == (4, {"noise": 37, "dropout": 40, "outliers": 40}[tag])
    out, ev = R.augment(x, points, _zeros(4), q, se, ss)
    assert ev["hit"].all()
    if tag == "dropout":
        assert torch.equal(out, y) and 0 < ev["drop"].sum() < ev["drop"].size and ev["exempt"].any() and not ev["exempt"].all()
        return
    assert R.check(y, x, points, q, ev, out) <= 1.0
    if tag == "noise":
        assert 0 < ev["mask"].sum() < ev["mask"].size and float((y - x).abs().max()) > 5e-4
    else:
        idx = G["outliers/index"]
        assert np.array_equal(ev["index"][:, :4], idx) and ev["replaced"].sum() == 16     # unique per cloud
        assert ev["contour"][:, :4].any() and not ev["contour"][:, :4].all()
        changed = (y != x).any(-1).numpy()
        assert np.array_equal(changed, ev["replaced"])


# ---- apply -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("points", [[37], [5, 37, 300], [1], [40, 40]])
def test_apply_float64_matches_the_restatement(points):
    N = 7
    x, ep = _cloud(N, points), torch.tensor([0, 1, 2, 0, 0, 5, 7], dtype=torch.int32)
    a = _P().PclAugment(points, seed=3, **ALL_ON)
    y = a.apply(x, ep, 12345678901234567)
    out, ev = R.augment(x, points, ep, a.params(), a.seed_episode, 12345678901234567)
    assert y.shape == x.shape and y.dtype == torch.float64
    assert float((y - out).abs().max()) <= 1e-12
    assert ev["hit"].any() and not ev["hit"].all()
    y3 = a.apply(x.reshape(N, -1, 3), ep, 12345678901234567)          # the other layout
    assert y3.shape == (N, sum(points), 3) and torch.equal(y3.reshape(x.shape), y)


@pytest.mark.parametrize("kw", [dict(), dict(rot_deg=30.0), dict(outlier_ratio=0.1), dict(dropout_ratio=0.2, no_dropout_prob=0.3),
                                ALL_ON], ids=["noise", "rotation", "outliers", "dropout", "all"])
def test_apply_fp32_is_within_the_bounds(kw):
    points, N = [37, 300], 9
    x, ep = _cloud(N, points, seed=1, dtype=torch.float32), torch.arange(N, dtype=torch.int32)
    a = _P().PclAugment(points, seed=5, **{"hit_prob": 0.8, **kw})
    y = a.apply(x, ep, 99)
    assert y.dtype == torch.float32
    out, ev = R.augment(x, points, ep, a.params(), a.seed_episode, 99)
    assert R.check(y, x, points, a.params(), ev, out) <= 1.0
    assert torch.equal(y[~torch.from_numpy(ev["hit"])], x[~torch.from_numpy(ev["hit"])])     # missed envs: bit for bit
    assert torch.equal((y.reshape(N, -1, 3) == 0).all(-1), torch.from_numpy(ev["drop"]))
    if kw.get("outlier_ratio"):
        far = ((y.double() - torch.from_numpy(ev["after_rot"]).reshape(x.shape)).abs() > 1e-4).reshape(N, -1, 3).any(-1)
        assert torch.equal(far | torch.from_numpy(ev["drop"]), torch.from_numpy(ev["replaced"] | ev["drop"]))


def test_duplicate_outlier_indices_the_highest_k_wins():
    points, N, seed = [40], 4, 5550001                                  # cloud 1 draws the indices 22, 19, 27, 19
    x = _cloud(N, points)
    a = _P().PclAugment(points, hit_prob=1.0, outlier_ratio=0.1, sigma=0.0, const_noise=0.0)
    out, ev = R.augment(x, points, _zeros(N), a.params(), a.seed_episode, seed)
    assert ev["index"][1, :4].tolist() == [22, 19, 27, 19]
    assert ev["winner"][1, 19] == 3 and ev["replaced"][1].sum() == 3
    y = a.apply(x, _zeros(N), seed).reshape(N, 40, 3)
    assert float((y - out.reshape(N, 40, 3)).abs().max()) <= 1e-12
    # the value of point 19 is outlier 3's, not outlier 1's: rebuild both from the draws
    e3, e1 = (40 + 3) * 3 + np.arange(3), (40 + 1) * 3 + np.arange(3)
    lo, hi = ev["after_rot"][1].min(0), ev["after_rot"][1].max(0)

    def outlier(k, e):
        if ev["contour"][1, k]:
            beyond = np.abs(R.gauss(seed, R.PLANE_CONTOUR, (N * 40 * 3,)).numpy()[e])
            return np.where(R.event(tok_hash(seed, R.SITE_SIDE, e), 0.5), hi + beyond, lo - beyond)
        return 1.5 * R.gauss(seed, R.PLANE_FREE, (N * 40 * 3,)).numpy()[e]
    assert np.allclose(y[1, 19].numpy(), outlier(3, e3), rtol=0, atol=1e-12)
    assert not np.allclose(y[1, 19].numpy(), outlier(1, e1), rtol=0, atol=1e-3)


def test_no_outliers_when_the_count_rounds_to_zero():
    points, N = [5], 6
    x = _cloud(N, points)
    P = _P()
    a, b = P.PclAugment(points, hit_prob=1.0, outlier_ratio=0.1), P.PclAugment(points, hit_prob=1.0)
    assert int(5 * 0.1) == 0
    assert torch.equal(a.apply(x, _zeros(N), 11), b.apply(x, _zeros(N), 11))
    _out, ev = R.augment(x, points, _zeros(N), a.params(), a.seed_episode, 11)
    assert not ev["replaced"].any()


def test_a_stage_that_is_off_changes_nothing():
    points, N = [37, 40], 5
    x = _cloud(N, points)
    P = _P()
    off = P.PclAugment(points, hit_prob=1.0, sigma=0.0, const_noise=0.0)
    assert torch.equal(off.apply(x, _zeros(N), 7), x)
    assert torch.equal(P.PclAugment(points, hit_prob=0.0, **{k: v for k, v in ALL_ON.items() if k != "hit_prob"})
                       .apply(x, _zeros(N), 7), x)
    base = P.PclAugment(points, hit_prob=1.0).apply(x, _zeros(N), 7)
    assert not torch.equal(base, x)
    # exempt clouds and a zero ratio: dropout leaves the noise-only result
    assert torch.equal(P.PclAugment(points, hit_prob=1.0, dropout_ratio=0.5, no_dropout_prob=1.0).apply(x, _zeros(N), 7), base)
    # no noise on any point (noise_prob 0) leaves only the per-env offset
    only_offset = P.PclAugment(points, hit_prob=1.0, noise_prob=0.0).apply(x, _zeros(N), 7).reshape(N, -1, 3)
    d = only_offset - x.reshape(N, -1, 3)
    assert float((d - d[:, :1]).abs().max()) < 1e-15 and float(d.abs().max()) <= R.f32(0.001)


def test_draw_is_private_and_seeded():
    P = _P()
    cpu_state = torch.get_rng_state()
    a, b, c = P.PclAugment([5], seed=4), P.PclAugment([5], seed=4), P.PclAugment([5], seed=5)
    sa, sb = [a.draw() for _ in range(5)], [b.draw() for _ in range(5)]
    assert sa == sb and len(set(sa)) == 5 and a.seed_episode == b.seed_episode != c.seed_episode
    assert all(0 <= s < 2 ** 63 for s in sa) and sa != [c.draw() for _ in range(5)]
    a.apply(_cloud(3, [5]), _zeros(3), sa[0])
    assert torch.equal(torch.get_rng_state(), cpu_state)


def test_event_frequencies():
    """>= 20,000 draws each; within 5 standard deviations of the nominal probability."""
    P = _P()
    n, seed = 24000, 31337

    def within(count, total, p):
        return abs(count - total * p) <= 5 * math.sqrt(total * p * (1 - p))
    points = [60, 60]
    a = P.PclAugment(points, hit_prob=0.7, rot_deg=10.0, outlier_ratio=0.5, dropout_ratio=0.2, no_dropout_prob=0.8, seed=1)
    _out, ev = R.augment(torch.zeros(200, 1, 360), points, _zeros(200), a.params(), a.seed_episode, seed)
    hits = int(ev["hit"].sum())
    assert within(int(ev["mask"].sum()), hits * 120, 0.3)               # 120 points per hit env: >= 20,000 at 0.7 x 200
    assert hits * 120 >= 12000
    assert within(int(ev["contour"].sum()), hits * 60, 0.75)
    # raw events over n draws: the same comparisons the stages make
    for site, p in ((R.SITE_HIT, 0.7), (R.SITE_MASK, 0.3), (R.SITE_DROP, 0.2), (R.SITE_CONTOUR, 0.75), (R.SITE_SIDE, 0.5)):
        assert within(int(R.event(tok_hash(seed, site, np.arange(n)), p).sum()), n, p), site
    exempt = ~R.event(tok_hash(seed, R.SITE_EXEMPT, np.arange(n)), R.f32(1.0 - 0.8))
    assert within(int(exempt.sum()), n, 0.8)
    axes = np.array([R.episode_params(a.seed_episode, env, 0, 10.0)[1] for env in range(n // 8)])   # 3000 envs ...
    from isaacgyminsertion_amd import draws
    ax = draws.index(draws.tok_hash(a.seed_episode, R.SITE_AXIS, torch.arange(n)), 3).numpy()       # ... and n through the hash
    assert np.array_equal(ax[:n // 8].astype(int), axes) and set(ax.tolist()) == {0, 1, 2}
    for k in range(3):
        assert within(int((ax == k).sum()), n, 1 / 3)


def test_episode_parameters_follow_the_episode_counter():
    P = _P()
    points, N = [37], 6
    x = _cloud(N, points)
    a = P.PclAugment(points, hit_prob=1.0, rot_deg=30.0, sigma=0.0, seed=2)
    ep = torch.tensor([0, 0, 3, 3, 9, 9], dtype=torch.int32)
    for env in range(N):
        p0 = R.episode_params(a.seed_episode, env, int(ep[env]), 30.0)
        p1 = R.episode_params(a.seed_episode, env, int(ep[env]), 30.0)
        p2 = R.episode_params(a.seed_episode, env, int(ep[env]) + 1, 30.0)
        assert p0[0] == p1[0] and p0[1] == p1[1] and np.array_equal(p0[2], p1[2])
        assert p0[0] != p2[0] and not np.array_equal(p0[2], p2[2]) and abs(p0[0]) <= 30.0
    # with sigma = 0 the result depends on the step seed only through the hit draw (1.0 here): two steps of one episode
    # agree, the next episode differs in every env
    y1, y2 = a.apply(x, ep, 100), a.apply(x, ep, 200)
    assert torch.equal(y1, y2)
    y3 = a.apply(x, ep + 1, 100)
    assert all(not torch.equal(y1[e], y3[e]) for e in range(N))
    ep2 = ep.clone()
    ep2[4] += 1
    y4 = a.apply(x, ep2, 100)
    assert torch.equal(y4[:4], y1[:4]) and torch.equal(y4[5], y1[5]) and not torch.equal(y4[4], y1[4])


# ---- the trainer's key --------------------------------------------------------------------------------------------------
def _engine(**env_keys):
    """An ``ExtrinsicAdapt`` on the host: everything but its optimizer (HIP only, not under test) is built."""
    from isaacgyminsertion_amd.algo.ext_adapt import ext_adapt
    from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
    from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
    from isaacgyminsertion_amd.utils.config import default_config
    pcl_info = env_keys.pop("pcl_info", True)
    randomize = env_keys.pop("randomize", None)
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu", obs_info=True, pcl_info=pcl_info)
    cfg.task.env.num_points, cfg.task.env.num_points_socket = 37, 40
    for k, v in env_keys.items():
        if v is _ABSENT:
            cfg.task.env.pop(k, None)
        else:
            cfg.task.env[k] = v
    if randomize is not None:
        cfg.task.randomize.update(randomize)
    env = SyntheticInsertionEnv(8, device="cpu", pcl_points=77 if pcl_info else 0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ext_adapt, "FlatAdam", lambda *a, **k: None)
        agent = ExtrinsicAdapt(env, None, cfg)
    agent.pcl_mean_std = agent.stud_obs_mean_std = lambda x: x      # the normalisers are HIP only, and not under test
    return agent, env


_ABSENT = object()


def test_default_config_has_the_keys_off():
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cpu")
    assert cfg.task.env.pcl_augment == "off" and cfg.task.env.PclProbNoise == 0.7
    assert dict(cfg.task.randomize) == dict(pcl_rot=30.0, pcl_rotate=False, pcl_outlier_ratio=0.0, pcl_dropout_ratio=0.0)


@pytest.mark.parametrize("key", [_ABSENT, "off"], ids=["absent", "off"])
def test_key_off_builds_no_augmentation(monkeypatch, key):
    calls = []
    monkeypatch.setattr(_P().PclAugment, "fused", lambda self, *a: calls.append(a))
    monkeypatch.setattr(_P().PclAugment, "__init__", lambda self, *a, **k: calls.append((a, k)))
    agent, env = _engine(pcl_augment=key)
    assert agent.pcl_augment is None and agent.pcl_episode is None and not calls
    obs = env.reset()
    a = agent.process_obs(obs, augment=True)["pcl"]
    assert torch.equal(a, obs["pcl"].reshape(8, -1, 3)) and not calls


def test_key_fused_builds_the_reference_live_augment():
    agent, _env = _engine(pcl_augment="fused")
    a = agent.pcl_augment
    assert isinstance(a, _P().PclAugment) and a.points == [37, 40]
    assert a.params() == R.params(hit_prob=0.7)                      # noise only
    assert agent.pcl_episode.dtype == torch.int32 and agent.pcl_episode.shape == (8,) and not agent.pcl_episode.any()
    agent, _env = _engine(pcl_augment="fused", PclProbNoise=0.5,
                          randomize=dict(pcl_rotate=True, pcl_rot=12.0, pcl_outlier_ratio=0.1, pcl_dropout_ratio=0.2))
    assert agent.pcl_augment.params() == R.params(hit_prob=0.5, rot_deg=12.0, outlier_ratio=0.1, dropout_ratio=0.2)
    b, _env = _engine(pcl_augment="fused")
    assert b.pcl_augment.seed_episode == a.seed_episode == _P().PclAugment([1], seed=42).seed_episode      # cfg.seed


def test_key_refusals():
    for bad in ("Fused", "on", "", True, 1):
        with pytest.raises(ValueError, match="task.env.pcl_augment"):
            _engine(pcl_augment=bad)
    with pytest.raises(ValueError, match="task.env.pcl_augment.*pcl_info"):
        _engine(pcl_augment="fused", pcl_info=False)


def test_process_obs_augments_only_when_asked(monkeypatch):
    agent, env = _engine(pcl_augment="fused")
    seen = []

    def fake(self, clouds, episode):
        seen.append((clouds, episode))
        return clouds + 1.0
    monkeypatch.setattr(_P().PclAugment, "fused", fake)
    obs = env.reset()
    plain = agent.process_obs(obs)["pcl"]
    assert not seen
    aug = agent.process_obs(obs, augment=True)["pcl"]
    assert len(seen) == 1 and seen[0][0].shape == obs["pcl"].shape and seen[0][1] is agent.pcl_episode
    assert aug.shape == plain.shape and not torch.equal(aug, plain)


# ---- the op --------------------------------------------------------------------------------------------------------------
def _op_args(N=3, points=(5, 7)):
    return dict(clouds=torch.zeros(N, 1, sum(points) * 3), points=list(points), episode=torch.zeros(N, dtype=torch.int32),
                params=R.params(), seed_episode=1, seed_step=2)


SCHEMA = ("mi355ppo::pcl_augment(Tensor clouds, int[] points, Tensor episode, float[] params, int seed_episode, "
          "int seed_step) -> Tensor")


def test_op_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "pcl_augment" in ops.OP_NAMES
    assert str(torch.ops.mi355ppo.pcl_augment.default._schema) == SCHEMA
    with FakeTensorMode():
        y = torch.ops.mi355ppo.pcl_augment(*_op_args().values())
        assert y.shape == (3, 1, 36) and y.dtype == torch.float32
        y = torch.ops.mi355ppo.pcl_augment(*{**_op_args(), "clouds": torch.zeros(3, 12, 3)}.values())
        assert y.shape == (3, 12, 3)


def test_c_abi_python_binding_and_cpp_registration_agree():
    from isaacgyminsertion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "igi_ppo.h")).read()
    capi = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "igi_capi.hip")).read()
    cpp = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "torch_ops.cpp")).read()
    kern = open(os.path.join(ROOT, "isaacgyminsertion_amd", "csrc", "pcl_augment.h")).read()
    assert "igi_pcl_augment" in _lib.exported_symbols()
    assert re.search(r"^int igi_pcl_augment\(", hdr, re.M) and re.search(r"^int igi_pcl_augment\(", capi, re.M)
    assert f"#define IGI_PCL_AUG_MAX_POINTS {ops.PCL_AUG_MAX_POINTS}" in hdr
    assert f"PCL_MAX_POINTS = {ops.PCL_AUG_MAX_POINTS};" in kern and f"PCL_MAX_OBJECTS = {ops.PCL_AUG_MAX_OBJECTS};" in kern
    decl = re.search(r"^int igi_pcl_augment\((.*?)\);", hdr, re.M | re.S).group(1)
    assert len(_lib._EXPORTS["igi_pcl_augment"][1]) == len(decl.split(",")) == 10
    assert "uint64_t seed_episode" in decl and "uint64_t seed_step" in decl
    struct = re.search(r"typedef struct igi_pcl_augment_params \{(.*?)\}", hdr, re.S).group(1)
    fields = [f.strip() for f in struct.replace("double", "").replace(";", "").split(",")]
    assert tuple(fields) == tuple(n for n, _t in _lib.PclAugmentParams._fields_) == tuple(ops.PCL_AUG_PARAMS) == R.ORDER
    schema = SCHEMA.replace("mi355ppo::", "")
    assert f'm.def("{schema}");' in cpp and 'm.impl("pcl_augment", pcl_augment);' in cpp


def _q(**kw):
    return dict(params=R.params(**kw))


@pytest.mark.parametrize("change, message", [
    (dict(clouds=torch.zeros(3, 1, 36, dtype=torch.float64)), "clouds: expected dtype"),
    (dict(clouds=torch.zeros(3, 36)), "clouds: expected 3 dimensions"),
    (dict(clouds=torch.zeros(3, 3, 12).transpose(1, 2)), "clouds: expected a contiguous"),
    (dict(episode=torch.zeros(3, dtype=torch.int64)), "episode: expected dtype"),
    (dict(episode=torch.zeros(3, 1, dtype=torch.int32)), "episode: expected 1 dimensions"),
    (dict(episode=torch.zeros(6, dtype=torch.int32)[::2]), "episode: expected a contiguous"),
    (dict(episode=torch.zeros(4, dtype=torch.int32)), "episode: expected shape"),
    (dict(points=[]), r"points: expected 1..4 objects"),
    (dict(points=[2, 2, 2, 2, 4]), r"points: expected 1..4 objects"),
    (dict(points=[0, 12]), r"points\[0\]: expected 1..4096"),
    (dict(points=[5, 4097], clouds=torch.zeros(1, 1, 4102 * 3), episode=torch.zeros(1, dtype=torch.int32)),
     r"points\[1\]: expected 1..4096"),
    (dict(points=[5, 6]), r"clouds: expected \(N, 1, 33\) or \(N, 11, 3\)"),
    (dict(clouds=torch.zeros(3, 2, 18)), r"clouds: expected \(N, 1, 36\) or \(N, 12, 3\)"),
    (dict(params=R.params()[:-1]), "params: expected 11 values"),
    (_q(hit_prob=1.01), r"hit_prob: expected a value in \[0, 1\]"),
    (_q(noise_prob=-0.1), r"noise_prob: expected a value in \[0, 1\]"),
    (_q(contour_prob=2.0), r"contour_prob: expected a value in \[0, 1\]"),
    (_q(no_dropout_prob=float("nan")), r"no_dropout_prob: expected a value in \[0, 1\]"),
    (_q(outlier_ratio=-0.5), r"outlier_ratio: expected a value in \[0, 1\]"),
    (_q(dropout_ratio=1.5), r"dropout_ratio: expected a value in \[0, 1\]"),
    (_q(sigma=-0.001), "sigma: expected >= 0"),
    (_q(noise_clip=-1.0), "noise_clip: expected >= 0"),
    (_q(rot_deg=-30.0), "rot_deg: expected >= 0"),
    (dict(clouds=torch.empty(2 ** 20, 1, 4096 * 3, device="meta"), points=[4096],
          episode=torch.empty(2 ** 20, dtype=torch.int32, device="meta")), "fewer than 2\\^32 coordinates"),
    (dict(), "expected a HIP"),                                   # everything else right, host tensors: no CPU path
])
def test_op_refuses_bad_arguments(change, message):
    args = {**_op_args(), **change}
    # 2^32 coordinates exist on no test host: that case hands storage-less tensors to the op's own function (the
    # dispatcher would send them to the fake kernel); every check before the launch reads shapes and dtypes only
    fn = ops.pcl_augment if args["clouds"].device.type == "meta" else torch.ops.mi355ppo.pcl_augment
    with pytest.raises(RuntimeError, match=message):
        fn(*args.values())
