"""The frozen actor on [obs | student latent] on the device (ActorCriticSplit.act_inference / act_with_grad with a
``latent`` entry: csrc/policy_fwd.h k_actor_latent at the reference's layer sizes, the actor's layers one launch each
otherwise; csrc/teacher.h teacher_actor_latent_forward / _backward) against float64 restatements
(tests/latent_student_ref.py) and against the chain of native Linear ops that ``_actor_critic_from_latent`` still runs.

Tolerances: mu and the saved activations at the project's inference bounds (tests/test_gpu_shared_critic.py: atol 2e-6,
rtol 1e-4); fused against layer by layer 2e-6 absolute and relative (tests/test_gpu_rollout.py, persistent against
layerwise); d/d latent at the step-0 gradient bound (1e-4 of the largest entry + 1e-3 relative).  Shapes: every row count
around a 32-row block (1, 31, 32, 33), three blocks with a ragged last (70), three chunks of an engine's 128 rows with
a ragged last (300), xcat with column 31 live (obs 24 + 8), other widths inside the gate (obs 9, latent 5, 3 actions; 7
actions), a shared trunk, and layer sizes outside the gate."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import latent_student_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULT = dict(obs=15, L=8, act=6, units=(512, 256, 128), shared=False, mb=None)
SHAPES = {
    "rows1": dict(DEFAULT, rows=1), "rows31": dict(DEFAULT, rows=31), "rows32": dict(DEFAULT, rows=32),
    "rows33": dict(DEFAULT, rows=33), "rows70": dict(DEFAULT, rows=70),
    "rows300_mb128": dict(DEFAULT, rows=300, mb=128),
    "obs24": dict(DEFAULT, rows=37, obs=24),
    "obs9_L5_act3": dict(DEFAULT, rows=37, obs=9, L=5, act=3),
    "act7": dict(DEFAULT, rows=37, act=7),
    "shared": dict(DEFAULT, rows=37, shared=True),
    "units48_40_24_L12": dict(DEFAULT, rows=37, units=(48, 40, 24), L=12),
}
GATED = [k for k, v in SHAPES.items() if v["units"] == (512, 256, 128)]
# a shared trunk under the adaptive learning-rate schedule: one more int behind the shared pair in the packed cfg
SHARED_ADAPTIVE = dict(DEFAULT, rows=33, shared=True, mb=128, lr_schedule="adaptive")
_CACHE = {}


def _case(name):
    """(net, obs, latent, dmu, float64 reference) of a shape, built once and left unchanged."""
    if name in _CACHE:
        return _CACHE[name]
    from isaacgyminsertion_amd.algo.models.models_split import ActorCriticSplit
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    s = SHARED_ADAPTIVE if name == "shared_adaptive" else SHAPES[name]
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    # the initialisation draws from the GLOBAL generator: seeded too, or every process tests another network (the fused
    # against chain comparison then moved between 2.9e-6 and 3.8e-6 at 300 rows from run to run, around its bound)
    torch.manual_seed(sum(ord(c) for c in name))
    net = ActorCriticSplit({'actions_num': s["act"], 'input_shape': (s["obs"],), 'actor_units': list(s["units"]),
                            'priv_mlp_units': [256, 128, s["L"]], 'priv_info': True, 'priv_info_dim': 64,
                            'shared_parameters': s["shared"]})
    with torch.no_grad():       # O(1) actions and non-zero biases (the initialisation has mu at std 0.01 and zero biases)
        net.mu.weight.copy_(torch.randn(net.mu.weight.shape, generator=g) * 0.3)
        for n, p in net.named_parameters():
            if n.endswith(".bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
    net = net.to(DEV)
    if s["mb"]:
        eng = TeacherEngine(s["mb"], 1, 1, units=list(s["units"]), priv_units=[256, 128, s["L"]], obs_dim=s["obs"],
                            priv_dim=64, act_dim=s["act"], device=DEV, lr_schedule=s.get("lr_schedule", "fixed"),
                            **net.engine_kwargs())
        net.bind_flat_to(eng)
        net.attach_engine(eng)
    obs = torch.randn(s["rows"], s["obs"], generator=g)
    lat = torch.randn(s["rows"], s["L"], generator=g)
    dmu = torch.randn(s["rows"], s["act"], generator=g)
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    lat64 = lat.double().requires_grad_(True)
    mu64 = lr.actor_mu(sd, obs.double(), lat64)
    mu64.backward(dmu.double())
    ref = dict(mu=mu64.detach(), dlatent=lat64.grad.detach(),
               hs=[h.detach() for h in lr.actor_activations(sd, obs.double(), lat64.detach())])
    _CACHE[name] = (net, obs.to(DEV), lat.to(DEV), dmu.to(DEV), ref)
    return _CACHE[name]


def _classes(fn):
    """{profiler class: launches} of fn()"""
    from isaacgyminsertion_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    return out, classes


def _split_saved(saved, units):
    out, col = [], 0
    for u in units:
        out.append(saved[:, col:col + u])
        col += (u + 3) & ~3
    assert col == saved.shape[1]
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_matches_float64(name):
    net, obs, lat, _, ref = _case(name)
    mu, latent = net.act_inference({'obs': obs, 'latent': lat})
    assert latent is lat and mu.shape == ref["mu"].shape and not mu.requires_grad
    err = (mu.cpu().double() - ref["mu"]).abs().max().item()
    print(f"{name}: max |mu - float64| = {err:.3e} (largest |mu| {ref['mu'].abs().max().item():.3f})")
    np.testing.assert_allclose(mu.cpu().numpy(), ref["mu"].numpy(), atol=2e-6, rtol=1e-4)


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_matches_the_layer_by_layer_chain(name):
    """the parent's path: cat + the native Linear + Tanh ops + the head ops, which actor_critic() still runs with a latent"""
    net, obs, lat, _, _ = _case(name)
    mu, _ = net.act_inference({'obs': obs, 'latent': lat})
    with torch.no_grad():
        mu_chain = net.actor_critic({'obs': obs, 'latent': lat})[0]
    print(f"{name}: max |fused - chain| = {(mu - mu_chain).abs().max().item():.3e}")
    np.testing.assert_allclose(mu.cpu().numpy(), mu_chain.cpu().numpy(), atol=2e-6, rtol=2e-6)


@pytest.mark.parametrize("rows", [1, 33, 70])
def test_ragged_stores_stay_inside_the_rows(rows):
    """igi_actor_latent_forward through ctypes, mu and hsave 40 rows longer than ``rows`` and filled with a sentinel"""
    from isaacgyminsertion_amd import _lib, ops
    net, _, _, _, _ = _case("rows70")
    eng = net._infer_engine(torch.device(DEV))
    cfg, st, _ = ops._teacher_args(eng.state_list(), *eng._cfg_args())
    g = torch.Generator().manual_seed(rows)
    obs, lat = torch.randn(rows, 15, generator=g).to(DEV), torch.randn(rows, 8, generator=g).to(DEV)
    S = _lib.lib().igi_actor_latent_saved_width(C.byref(cfg))
    assert S == 896
    sentinel = -123.25
    mu = torch.full((rows + 40, 6), sentinel, device=DEV)
    hsave = torch.full((rows + 40, S), sentinel, device=DEV)
    rc = _lib.lib().igi_actor_latent_forward(C.byref(cfg), C.byref(st), _lib.ptr(obs), _lib.ptr(lat), 8, rows, _lib.ptr(mu),
                                             _lib.ptr(hsave), _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((mu[rows:] == sentinel).all()) and bool((hsave[rows:] == sentinel).all())
    assert bool((mu[:rows] != sentinel).all()) and bool((hsave[:rows] != sentinel).all())
    want, _ = eng.actor_latent(obs, lat, False)
    assert torch.equal(mu[:rows], want)
    # a latent of another width than the teacher's extrinsic is refused, nothing is written
    assert _lib.lib().igi_actor_latent_forward(C.byref(cfg), C.byref(st), _lib.ptr(obs), _lib.ptr(lat), 7, rows, _lib.ptr(mu),
                                               None, _lib.current_stream(torch.device(DEV))) != 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_saved_activations_and_backward_match_float64(name):
    net, obs, lat, dmu, ref = _case(name)
    eng = net._infer_engine(torch.device(DEV))
    mu, saved = eng.actor_latent(obs, lat, True)
    assert saved.shape == (obs.shape[0], sum((u + 3) & ~3 for u in SHAPES[name]["units"]))
    for l, (h, h64) in enumerate(zip(_split_saved(saved, SHAPES[name]["units"]), ref["hs"])):
        np.testing.assert_allclose(h.cpu().numpy(), h64.numpy(), atol=2e-6, rtol=1e-4, err_msg=f"h{l + 1}")
    dlat = eng.actor_latent_backward(saved, dmu)
    r = ref["dlatent"].numpy()
    print(f"{name}: max |dlatent - float64| = {np.abs(dlat.cpu().numpy() - r).max():.3e} of {np.abs(r).max():.3e}")
    np.testing.assert_allclose(dlat.cpu().numpy(), r, atol=1e-4 * np.abs(r).max(), rtol=1e-3)
    # through autograd: the same gradient in the latent, none in a teacher parameter, none in the observation
    lat_g = lat.clone().requires_grad_(True)
    mu_g, latent = net.act_with_grad({'obs': obs, 'latent': lat_g})
    assert latent is lat_g and mu_g.requires_grad and torch.equal(mu_g.detach(), mu)
    mu_g.backward(dmu)
    assert torch.equal(lat_g.grad, dlat)
    assert all(p.grad is None for p in net.parameters())
    # no graph without a latent that asks for one, or under no_grad
    assert not net.act_with_grad({'obs': obs, 'latent': lat})[0].requires_grad
    with torch.no_grad():
        assert not net.act_with_grad({'obs': obs, 'latent': lat_g})[0].requires_grad


def test_shared_trunk_under_the_adaptive_schedule_matches_float64():
    """forward with saved activations, then the backward, at 33 rows: the bounds of the test above, and d/d latent as
    wide as the teacher's extrinsic"""
    net, obs, lat, dmu, ref = _case("shared_adaptive")
    eng = net._infer_engine(torch.device(DEV))
    assert eng.cfg.lr_schedule == 1 and eng.cfg.shared_parameters == 1
    mu, saved = eng.actor_latent(obs, lat, True)
    assert saved.shape == (33, 512 + 256 + 128)
    np.testing.assert_allclose(mu.cpu().numpy(), ref["mu"].numpy(), atol=2e-6, rtol=1e-4)
    for l, (h, h64) in enumerate(zip(_split_saved(saved, DEFAULT["units"]), ref["hs"])):
        np.testing.assert_allclose(h.cpu().numpy(), h64.numpy(), atol=2e-6, rtol=1e-4, err_msg=f"h{l + 1}")
    dlat = eng.actor_latent_backward(saved, dmu)
    assert dlat.shape == (33, DEFAULT["L"])
    r = ref["dlatent"].numpy()
    np.testing.assert_allclose(dlat.cpu().numpy(), r, atol=1e-4 * np.abs(r).max(), rtol=1e-3)


def test_launches():
    gemm = lambda classes: {k: v for k, v in classes.items() if k.startswith("gemm_") and v}   # noqa: E731
    net, obs, lat, _, _ = _case("rows70")
    net.act_inference({'obs': obs, 'latent': lat})          # (the engine exists, its kernels are loaded)
    _, classes = _classes(lambda: net.act_inference({'obs': obs, 'latent': lat}))
    print("act_inference(latent), 70 rows:", classes)
    assert classes.get("k_actor_latent", 0) == 1 and not gemm(classes), classes
    assert sum(classes.values()) == 2, classes               # + the refresh of the padded first-layer mirror
    lat_g = lat.clone().requires_grad_(True)
    (mu, _), classes = _classes(lambda: net.act_with_grad({'obs': obs, 'latent': lat_g}))
    print("act_with_grad(latent), 70 rows:", classes)
    assert classes.get("k_actor_latent", 0) == 1 and not gemm(classes) and mu.grad_fn is not None, classes
    _, classes = _classes(lambda: mu.sum().backward())
    print("its backward:", classes)
    assert classes.get("k_actor_latent", 0) == 0 and sum(gemm(classes).values()) == 3, classes
    # three chunks of an engine with 128-row minibatches: one launch each
    net3, obs3, lat3, _, _ = _case("rows300_mb128")
    _, classes = _classes(lambda: net3.act_inference({'obs': obs3, 'latent': lat3}))
    assert classes.get("k_actor_latent", 0) == 3 and not gemm(classes), classes
    # a shared trunk takes the kernel too; layer sizes off the gate do not
    nets, obss, lats, _, _ = _case("shared")
    _, classes = _classes(lambda: nets.act_inference({'obs': obss, 'latent': lats}))
    assert classes.get("k_actor_latent", 0) == 1 and not gemm(classes), classes
    neto, obso, lato, _, _ = _case("units48_40_24_L12")
    _, classes = _classes(lambda: neto.act_inference({'obs': obso, 'latent': lato}))
    print("units 48 / 40 / 24:", classes)
    assert classes.get("k_actor_latent", 0) == 0 and sum(gemm(classes).values()) == 3, classes


@pytest.mark.parametrize("name", ["rows70", "rows300_mb128", "units48_40_24_L12"])
def test_two_calls_give_the_same_bits(name):
    net, obs, lat, dmu, _ = _case(name)
    eng = net._infer_engine(torch.device(DEV))
    mu_a, saved_a = eng.actor_latent(obs, lat, True)
    d_a = eng.actor_latent_backward(saved_a, dmu)
    mu_b, saved_b = eng.actor_latent(obs, lat, True)
    d_b = eng.actor_latent_backward(saved_b, dmu)
    assert torch.equal(mu_a, mu_b) and torch.equal(saved_a, saved_b) and torch.equal(d_a, d_b)
    assert torch.equal(eng.actor_latent(obs, lat, False)[0], mu_a)
