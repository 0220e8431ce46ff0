"""igi_depth_forward / igi_depth_backward (DepthOnlyFCBackbone54x96) against the golden captured from the
reference's own module (tests/golden/depth.npz; weights / inputs regenerated from the generator's seeds), and
against ATen fp64 on other batch sizes.  Tolerances: fp32 network with reductions of up to 64768 (fc1) and
32 x 1150 (conv1 weight gradient) terms: outputs 2e-5 x max|y|; gradients 2e-4 x the tensor's largest entry."""
import os
import sys

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
from oracle import encoders as oe  # noqa: E402
from make_golden_depth import depth_case  # noqa: E402  (seeded inputs only; the reference is not imported)

pytestmark = pytest.mark.gpu


def _module(sd, latent=32):
    from isaacgyminsertion_amd.algo.models.transformer.depth_backbone import DepthOnlyFCBackbone54x96
    m = DepthOnlyFCBackbone54x96(latent_dim=latent)
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda()


def _close(name, got, want, rel):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    assert err <= rel * np.abs(want).max() + 1e-7, (name, err, np.abs(want).max())


def test_matches_reference_module():
    G = load_golden("depth.npz")
    sd, x, dy = depth_case()
    m = _module(sd)
    y = m(x.cuda())
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    _close("y", y.detach().cpu().numpy(), G["y"], 2e-5)
    for k, p in m.named_parameters():
        g = p.grad.cpu().numpy()
        if k == "image_compression.6.weight":
            _close(k + "/sample", g[::8, ::997], G["g/" + k + "/sample"], 2e-4)
            _close(k + "/rowsum", g.sum(1), G["g/" + k + "/rowsum"], 2e-4)
            _close(k + "/colsum", g.sum(0), G["g/" + k + "/colsum"], 2e-4)
        else:
            _close(k, g, G["g/" + k], 2e-4)


def _aten(sd, x, dy):
    """ATen fp64 on the CPU: oracle/encoders.py:depth_backbone (pinned to depth.npz by tests/test_oracle_encoders.py)"""
    return oe.value_and_grads(oe.depth_backbone, x, sd, dy, dtype=torch.float64)


@pytest.mark.parametrize("batch,latent", [(64, 32), (5, 8), (33, 32), (96, 4), (128, 64)])
def test_matches_aten_other_shapes(batch, latent):
    """incl. batches that are not a multiple of 32 (padded inside the op); 96: three 32-image groups in the conv2
    weight-gradient walk and the first wrap of the fc1 weight gradient's two-stage ring, with the narrowest head the plan
    accepts (4); 128: the largest batch still on 128-row convolution tiles."""
    sd, x, dy = depth_case(latent=latent, batch=batch, seed=batch)
    m = _module(sd, latent)
    y = m(x.cuda())
    y.backward(dy.cuda())
    yr, gr = _aten(sd, x, dy)
    _close("y", y.detach().cpu().numpy(), yr.numpy(), 2e-5)
    for k, p in m.named_parameters():
        _close(k, p.grad.cpu().numpy(), gr[k].numpy(), 2e-4)


def test_backward_is_deterministic_and_input_gets_no_grad():
    sd, x, dy = depth_case(batch=32, seed=3)
    m = _module(sd)
    xs = x.cuda().requires_grad_(True)
    outs = []
    for _ in range(2):
        m.zero_grad()
        y = m(xs)
        y.backward(dy.cuda())
        outs.append([p.grad.clone() for p in m.parameters()])
    assert xs.grad is None
    for a, b in zip(*outs):
        assert torch.equal(a, b)
