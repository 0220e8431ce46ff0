"""CPU: oracle/encoders.py (PyTorch-CPU restatement of the reference's CNNWithSpatialSoftArgmax / PointNet) against
golden vectors produced by the reference's own modules (tests/golden/make_golden_encoders.py).  fp32 run: outputs
1e-6 abs + 1e-5 rel, gradients 2e-5 * max|g| (same ATen kernels as the reference, so nearly bit-equal); the fp64
run measures the reference's own fp32 rounding: <= 1.1e-4 of a tensor's largest gradient entry at 32 x 64, up to
4.5e-3 at 64 x 64 (the soft-argmax gradient sums to zero over 576 positions, so the conv gradients under it cancel
heavily) -- the yardstick the HIP tests at scale use (error against fp64 <= 3 x the fp32 oracle's own error).
The depth backbone (oe.depth_backbone) is pinned the same way to tests/golden/depth.npz, at 1e-5 of each tensor's largest
entry (both sides are the same ATen calls in fp32)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import encoders as oe

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "encoders.npz"))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_depth import depth_case  # noqa: E402  (seeded inputs only; the reference is not imported)


def _case(tag):
    sd = {k[len(tag) + 3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/p/")}
    return sd, torch.from_numpy(G[f"{tag}/x"]), torch.from_numpy(G[f"{tag}/gy"])


@pytest.mark.parametrize("tag,fn", [("tac32x64", oe.tactile_cnn), ("tac64x64", oe.tactile_cnn), ("tac_b5", oe.tactile_cnn),
                                    ("pn400", oe.pointnet), ("pn37", oe.pointnet)])
def test_encoder_oracle_matches_reference_golden(tag, fn):
    torch.set_num_threads(1)
    sd, x, gy = _case(tag)
    y, g = oe.value_and_grads(fn, x, sd, gy)
    np.testing.assert_allclose(y.numpy(), G[f"{tag}/y"], atol=1e-6, rtol=1e-5)
    for k in sd:
        ref = G[f"{tag}/g/{k}"]
        np.testing.assert_allclose(g[k].numpy(), ref, atol=2e-5 * np.abs(ref).max(), rtol=1e-4, err_msg=k)
    # fp64 rerun, evaluated in two chunks (the functional is additive over samples): the reference's fp32 rounding
    y64, g64 = oe.value_and_grads(fn, x, sd, gy, dtype=torch.float64, chunk=(x.shape[0] + 1) // 2)
    np.testing.assert_allclose(y64.numpy(), G[f"{tag}/y"], atol=2e-5, rtol=1e-4)
    for k in sd:
        ref = G[f"{tag}/g/{k}"]
        np.testing.assert_allclose(g64[k].numpy(), ref, atol=1e-2 * np.abs(ref).max(), rtol=1e-2, err_msg=k)


def test_softargmax_oracle_matches_reference_golden():
    S = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softargmax.npz"))
    for tag in ("n_8x24", "n_24x24", "i_10x26", "n_1ch"):
        x = torch.from_numpy(S[f"{tag}/x"]).requires_grad_()
        y = oe.spatial_softargmax(x, bool(S[f"{tag}/normalize"]))
        (y * torch.from_numpy(S[f"{tag}/gy"])).sum().backward()
        np.testing.assert_allclose(y.detach().numpy(), S[f"{tag}/y"], atol=1e-6, rtol=1e-6, err_msg=tag)
        np.testing.assert_allclose(x.grad.numpy(), S[f"{tag}/gx"], atol=1e-7, rtol=1e-5, err_msg=tag)


def _within(name, got, want, rel):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    assert err <= rel * np.abs(want).max(), f"{name}: err {err:.3e}, largest entry {np.abs(want).max():.3e}"


def test_depth_oracle_matches_reference_golden():
    """oe.depth_backbone in fp32 on depth_case() against what the reference's DepthOnlyFCBackbone54x96 computed from the
    same seeds (depth.npz): the output, every small gradient, and the sample / row sums / column sums of the 128 x 64768
    fc1 weight gradient, each within 1e-5 of the tensor's largest entry."""
    D = np.load(os.path.join(HERE, "golden", "depth.npz"))
    sd, x, dy = depth_case()
    y, g = oe.value_and_grads(oe.depth_backbone, x, sd, dy)
    assert list(g.keys()) == list(sd.keys())
    _within("y", y.numpy(), D["y"], 1e-5)
    for k in sd:
        gk = g[k].numpy()
        if k == "image_compression.6.weight":
            _within(k + "/sample", gk[::8, ::997], D["g/" + k + "/sample"], 1e-5)
            _within(k + "/rowsum", gk.sum(1), D["g/" + k + "/rowsum"], 1e-5)
            _within(k + "/colsum", gk.sum(0), D["g/" + k + "/colsum"], 1e-5)
        else:
            _within(k, gk, D["g/" + k], 1e-5)
    # chunked evaluation (the functional is additive over samples) is the same gradient; other batch sizes change
    # ATen's blocking of the fp32 sums, so the two agree to fp32 rounding (the bound above), not to the bit
    y2, g2 = oe.value_and_grads(oe.depth_backbone, x, sd, dy, chunk=13)
    _within("y, chunked", y2.numpy(), y.numpy(), 1e-5)
    for k in sd:
        _within(k + ", chunked", g2[k].numpy(), g[k].numpy(), 1e-5)


def test_depth_pool_near_ties_marks_near_ties_and_not_exact_ones():
    """A constant image makes every pool window an exact tie (all four pre-pool values are the same sum): not marked.
    Raising one pixel by 1e-7 moves window values apart by |w| * 1e-7 < 5e-7: marked; raising it by 1e-2 is a clear
    maximum (gap |w| * 1e-2, and w != 0): that image is not marked by ITS pixel -- checked with a single-tap kernel."""
    sd, _, _ = depth_case()
    w = torch.zeros(32, 1, 5, 5)
    w[:, 0, 0, 0] = 1.0                      # conv1 = the top-left pixel of each patch + bias
    sd = dict(sd, **{"image_compression.0.weight": w})
    x = torch.full((3, 1, 54, 96), 0.5, dtype=torch.float64)
    x[1, 0, 10, 10] += 1e-7
    x[2, 0, 10, 10] += 1e-2
    assert oe.depth_pool_near_ties(x, sd).tolist() == [False, True, False]
    assert oe.depth_pool_near_ties(x, sd, thr=1e-8).tolist() == [False, False, False]
