"""The student with an observation history (``context_size`` = ``sequence_length`` > 1) against golden vectors from the
reference's own ``MultiModalModel`` (tests/golden/make_golden_student_seq.py): the per-step reshape / transpose of the
tactile encodings with its (context, batch) order, the 3-D ``lin_input``, the positional encoding over context x
modalities tokens, the token transformer beyond 8 tokens (k_token_fwd_long / the tile attention kernels) and the
``Linear(S * 32, 32)`` output stack.  Dropout off, as in the golden run.

Bounds: those test_gpu_student.py applies to its reference cases -- gradients per tensor 1e-3 of the largest entry (+ 1e-3
relative), or 4 x the reference's own recorded fp32-vs-float64 distance where that is larger.  test_gpu_student.py has no
bound on the output to inherit (it compares per-step action losses at 2e-4 relative, which these cases do not have), so
the output's bound is this file's own, and tighter than that one: the output (a Tanh, at most
1 in size, of an fp32 chain through the same network) gets the absolute bound the token-encoder tests put on an O(1) fp32
output, 2e-5, or 4 x the reference's own recorded fp32-vs-float64 distance where that is larger.  Inputs are regenerated
from the generator's seeds, not stored."""
import numpy as np
import pytest
import torch

from tests.golden import make_golden_student_seq as mg

pytestmark = pytest.mark.gpu
G = mg.load()


def _model(tag):
    from isaacgyminsertion_amd.algo.models.transformer.tact import MultiModalModel
    context, tactile, B, seed = [int(v) for v in G[f"{tag}/flags"]]
    model = MultiModalModel(**mg.model_kwargs(context, bool(tactile)))
    assert [str(k) for k in G[f"{tag}/keys"]] == list(model.state_dict().keys())
    model.load_state_dict({k: torch.from_numpy(G[f"{tag}/init/{k}"]) for k in model.state_dict()})
    for m in model.modules():      # dropout RNG streams differ across devices: off, as in the golden run
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    return model.cuda().train(), mg.case_inputs(context, bool(tactile), B, seed)


@pytest.mark.parametrize("tag", [c[0] for c in mg.CASES])
def test_history_student_matches_the_reference(tag):
    model, (tac, lin, w) = _model(tag)
    context = int(G[f"{tag}/flags"][0])
    assert model.decoder.positional_encoding.pos_enc.shape[1] == context * (2 if tac is not None else 1) > 8
    y = model(None if tac is None else tac.cuda(), None, None, lin_input=lin.cuda())
    (y * w.cuda()).sum().backward()
    ref = G[f"{tag}/y"]
    err = np.abs(y.detach().cpu().numpy() - ref).max()
    print(f"[{tag}] y: err {err:.3e} max|y| {np.abs(ref).max():.3e} reference's own fp32 distance {float(G[f'{tag}/y_ref_noise']):.3e}")
    np.testing.assert_allclose(y.detach().cpu().numpy(), ref, rtol=0,
                               atol=max(2e-5, 4 * float(G[f"{tag}/y_ref_noise"])), err_msg="y")
    names = [k[len(tag) + 7:] for k in G if k.startswith(f"{tag}/grad0/")]
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert len(names) >= 20 and set(names) <= set(got), set(names) - set(got)
    gmax = max(np.abs(G[f"{tag}/grad0/{nm}"]).max() for nm in names)
    worst = 0.0
    for nm in names:
        ref = G[f"{tag}/grad0/{nm}"]
        noise = float(G[f"{tag}/grad0_ref_noise/{nm}"])
        atol = max(1e-3 * np.abs(ref).max(), 1e-6 * gmax, 4 * noise)
        worst = max(worst, float(np.abs(got[nm].cpu().numpy() - ref).max()) / atol)
    print(f"[{tag}] gradients: worst error {100 * worst:.1f} % of the absolute part of its bound")
    for nm in names:
        ref = G[f"{tag}/grad0/{nm}"]
        noise = float(G[f"{tag}/grad0_ref_noise/{nm}"])
        np.testing.assert_allclose(got[nm].cpu().numpy(), ref, atol=max(1e-3 * np.abs(ref).max(), 1e-6 * gmax, 4 * noise),
                                   rtol=1e-3, err_msg=f"grad0 {nm}")
    for nm, g in got.items():      # the never-called template layer (decoder.sa_layer.*) carries no gradient
        assert nm in names or float(g.abs().max()) == 0.0, nm


def test_runner_with_a_history_of_12_predicts_what_its_model_computes():
    """Runner(sequence_length=12), lin only: context_size 12 selects the transformer decoder over 12 tokens; predict
    returns the model's eval-mode output for the same frames, for 2-D (flattened history) and 3-D student_obs alike."""
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.algo.models.transformer.tact import MultiLayerDecoder
    from isaacgyminsertion_amd.utils.config import default_config
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cuda:0")
    cfg.offline_train.model.transformer.sequence_length = 12
    torch.manual_seed(0)
    runner = Runner(cfg)
    model = runner.model
    assert model.context_size == 12 and isinstance(model.decoder, MultiLayerDecoder)
    assert model.decoder.output_layers[0].in_features == 12 * 32
    with torch.no_grad():          # O(1)-scale weights so the outputs are not ~1e-6
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight)
    obs = torch.randn(8, 12, 15, generator=torch.Generator().manual_seed(1))
    out, _ = runner.predict({"student_obs": obs})
    assert out.shape == (8, 6) and torch.isfinite(out).all() and float(out.abs().max()) > 1e-2
    assert not model.training
    with torch.no_grad():
        want = model(None, None, None, lin_input=obs.cuda())
    assert torch.equal(out, want)
    out2, _ = runner.predict({"student_obs": obs.reshape(8, 12 * 15)})
    assert torch.equal(out2, want)
    # a frame matters where it stands: swapping two steps of the history changes the prediction
    swapped = obs.clone()
    swapped[:, [0, 11]] = obs[:, [11, 0]]
    out3, _ = runner.predict({"student_obs": swapped})
    assert not torch.allclose(out3, want, atol=1e-4)


def test_point_clouds_with_a_history_are_refused():
    from isaacgyminsertion_amd.algo.models.transformer.tact import MultiModalModel
    pcl_conf = {"num_sample_plug": 400, "num_sample_hole": 400, "num_sample_goal": 400, "num_sample_all": 400,
                "merge_socket": True, "merge_goal": False, "scene_pcl": False, "merge_plug": True, "relative": False}
    kw = mg.model_kwargs(4, False)
    kw.update(include_pcl=True, pcl_conf=pcl_conf)
    with pytest.raises(NotImplementedError, match="reference sizes the decoder"):
        MultiModalModel(**kw)
    kw["context_size"] = 1         # without a history the same modalities build
    assert MultiModalModel(**kw).context_size == 1
