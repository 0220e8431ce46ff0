"""The depth backbone (csrc/depth.h, DepthOnlyFCBackbone54x96) ABOVE 64 IMAGES, forward and backward, against fp64.

tests/test_gpu_depth.py and the student goldens stop at 64 images (128 from this file's companion shapes there).  Above
that the launch code of depth.h and the dispatcher of gemm_dma.h run other code:
  * conv2 forward (3x3 taps, C = 32, K = 288, N = 64, M = B * 1012) moves to the 256-row tile
    ``gemm_dma_kernel<64,true,true,1,2,256>`` from ceil(M / 256) >= 512, i.e. B >= 160; tiles straddle images;
  * conv2 data gradient (pad 2, 3x3, C = 64 -> 32, K = 576, M = B * 1150): the row-major tall tile
    ``<32,true,true,1,2,256>`` (out-of-image taps read the zero page) from 128 images, the position-major
    ``<32,true,true,4,2,256>`` (out-of-image taps skipped, epilogue row stride = one image) when B is a multiple of 256;
  * conv2 weight gradient (M = 288: three 128-row tap tiles, the last with 32 live rows; position-major reduction, split
    over k): 85 splits below 688 images, 170 from 688; 32-image group index 0 .. B / 32 - 1;
  * k_depth_conv1_wgrad runs min(B, 512) workgroups: above 512 images some loop over two images, others take one;
    k_depth_conv1_fwd runs min(B, 2048) workgroups, the second pass starts at image 2048;
  * fc1: weight gradient with K = B (two-stage ring), forward split-K factor chosen from B.
These tests run exactly those instantiations (asserted through the igi_prof_* class names and launch counts) on
``depth_case(32, B, seed=B)`` -- random images with a zeroed corner, so EXACT pooling ties are present -- and compare with
oracle/encoders.py:depth_backbone on the CPU (pinned to the reference's depth.npz by tests/test_oracle_encoders.py) in fp32
and fp64.  Bounds (test_gpu_depth.py's own): outputs within 2e-5 * max|y| of fp64, row by row; gradients per tensor
|hip - fp64| <= max(2e-4 * max|g|, 3 x |fp32 oracle - fp64|); against the sum of 64-image calls of the same module (the
instantiation depth.npz pins) 2e-4 * max|g|.

Max-pool is the network's only discontinuity of the gradient (ELU is C1).  Images in which some pool window's two largest
pre-pool values are 0 < gap < 5e-7 apart in fp64 (oracle/encoders.py:depth_pool_near_ties) carry no upstream gradient: which
one an fp32 sum calls the larger is not defined by the reference either.  Exact ties (the zeroed corner) stay in: the first
maximum wins everywhere.  At most 10 % of the images may be masked.

Measured on an MI355X (device error | the fp32 oracle's own error, both against fp64, as shares of max|g| resp. max|y|):
  tensor        160 images            768 images            768 images, dy on the six block-edge images
  y             8.3e-7 | 7.4e-7       1.0e-6 | 6.8e-7       6.4e-7 | 1.9e-6
  conv1 weight  6.8e-7 | 1.6e-6       7.2e-7 | 1.4e-6       5.3e-7 | 4.8e-7
  conv1 bias    4.1e-7 | 1.1e-6       9.1e-7 | 1.6e-6       6.4e-7 | 3.6e-7
  conv2 weight  1.2e-6 | 1.8e-6       1.2e-6 | 1.5e-6       4.5e-7 | 1.5e-6
  conv2 bias    1.1e-6 | 1.8e-6       1.2e-6 | 1.2e-6       3.6e-7 | 1.2e-6
  fc1 weight    8.3e-7 | 6.8e-7       9.2e-7 | 4.0e-7       5.3e-7 | 4.4e-7
  fc1 bias      3.9e-7 | 2.9e-7       4.8e-7 | 1.6e-7       2.5e-7 | 3.1e-7
  fc2 weight    3.8e-7 | 4.0e-7       4.8e-7 | 4.4e-7       6.8e-7 | 8.7e-7
  fc2 bias      1.4e-7 | 8.1e-8       2.4e-7 | 8.5e-8       4.9e-8 | 4.9e-8
2080 images, forward: rows 0 .. 31 and 2016 .. 2079 1.3e-6 of max|y| (fp32 oracle 6.8e-7); rows 2048 .. 2079 against a
32-image call 1.4e-6.  Images masked: 3.8 % at 160, 6.9 % at 768 (none of the six block-edge images).  Profiler classes
of one forward + backward: gemm_dma_kernel<128,true,true>, <128,true,false>, <128,false,false>, <64,true,true>,
<64,false,false> (one launch each: the two Linears and the 128-row tap tiles of conv2's weight gradient),
<64,true,true,1,2,256> (one), and <32,true,true,1,2,256> at 160 / <32,true,true,4,2,256> at 768 (one); the 64-image calls
launch none of the 256-row classes, and the one-launch gradient is within 1.4e-6 of max|g| of their sum (conv2 weight, both
batches).  A library whose k_depth_conv1_wgrad leaves out image 767 misses by 4.4e-2 of max|g| in the 768-image case and by
0.39 in the block-edge case.  No comparison failed: nothing in depth.h or gemm_dma.h had to change.
Not pinned: batches near the 32768 limit (the conv2 forward loader's switch away from 32-bit offsets at ~29,000 images and
the 2^31 guards): ~25 GB of workspace per call and a CPU reference of minutes.
"""
import ctypes as C
import functools
import sys

import numpy as np
import pytest
import torch

from golden_io import GOLDEN

sys.path.insert(0, GOLDEN)
from make_golden_depth import depth_case  # noqa: E402  (seeded inputs only; the reference is not imported)
from oracle import encoders as oe  # noqa: E402

pytestmark = pytest.mark.gpu

TALL_FWD_64 = "gemm_dma_kernel<64,true,true,1,2,256>"     # conv2 forward, 256-row tiles
TALL_DGRAD_32 = "gemm_dma_kernel<32,true,true,1,2,256>"   # conv2 data gradient, row-major 256-row tiles (zero-page taps)
PM_DGRAD_32 = "gemm_dma_kernel<32,true,true,4,2,256>"     # conv2 data gradient, position-major tiles (whole 256-image blocks)
EDGES = [0, 255, 256, 511, 512, 767]   # first / last image of each 256-image block; 511 | 512: the two passes of conv1's weight gradient


def _module(sd, latent=32):
    from isaacgyminsertion_amd.algo.models.transformer.depth_backbone import DepthOnlyFCBackbone54x96
    m = DepthOnlyFCBackbone54x96(latent_dim=latent)
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    return m.cuda()


def _profiled(fn):
    from isaacgyminsertion_amd import _lib
    _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    return out, classes


@functools.lru_cache(maxsize=None)
def _case(B):
    """(sd, x, dy, near-tie mask) of depth_case(32, B, seed=B); shared between tests, never written to"""
    sd, x, dy = depth_case(latent=32, batch=B, seed=B)
    return sd, x, dy, oe.depth_pool_near_ties(x, sd)


def _forward_backward(m, x, gy):
    m.zero_grad()
    y = m(x)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _assert_rows_close(name, y_hip, y64, y32=None):
    """every row within 2e-5 * max|y| of fp64"""
    ref = y64.numpy().astype(np.float64)
    scale = np.abs(ref).max()
    err_rows = np.abs(y_hip.cpu().numpy().astype(np.float64) - ref).max(axis=1)
    err_ref = np.abs(y32.numpy().astype(np.float64) - ref).max() if y32 is not None else float("nan")
    msg = f"{name}: |hip - fp64| = {err_rows.max():.3e} at row {int(err_rows.argmax())} = {err_rows.max() / scale:.2e} of " \
          f"max|y| = {scale:.3e} (fp32 oracle: {err_ref:.3e} = {err_ref / scale:.2e})"
    print(msg)
    assert err_rows.max() <= 2e-5 * scale, msg


def _assert_close_to_truth(name, hip, g32, g64):
    """per tensor: |hip - fp64| <= max(2e-4 * max|g|, 3 x |fp32 oracle - fp64|)"""
    ref = g64.numpy()
    scale = np.abs(ref).max()
    err_hip = np.abs(hip.cpu().numpy().astype(np.float64) - ref).max()
    err_ref = np.abs(g32.numpy().astype(np.float64) - ref).max()
    msg = f"{name}: |hip - fp64| = {err_hip:.3e} = {err_hip / scale:.2e} of max|g| = {scale:.3e} " \
          f"(fp32 oracle: {err_ref:.3e} = {err_ref / scale:.2e})"
    print(msg)
    assert err_hip <= max(2e-4 * scale, 3.0 * err_ref), msg


@pytest.mark.parametrize("B", [160, 768])
def test_depth_forward_backward_at_scale(B):
    """160: tall conv2 forward + the row-major tall data gradient (both with a partial last tile).  768 = 3 x 256: the
    position-major data gradient with image blocks 0, 1, 2, the 170-way conv2 weight-gradient split and the uneven second
    pass of k_depth_conv1_wgrad (256 of its 512 workgroups take two images)."""
    sd, x, dy, near = _case(B)
    share = float(near.float().mean())
    print(f"B = {B}: {100 * share:.1f} % of the images masked (pool near-ties)")
    assert share <= 0.10, share
    gy = dy.clone()
    gy[near] = 0.0
    xc, gyc = x.cuda(), gy.cuda()
    m = _module(sd)
    (y, grads), classes = _profiled(lambda: _forward_backward(m, xc, gyc))
    print(f"B = {B}: classes", classes)
    assert classes.get(TALL_FWD_64) == 1, classes
    if B == 160:
        assert classes.get(TALL_DGRAD_32) == 1 and PM_DGRAD_32 not in classes, classes
    else:
        assert classes.get(PM_DGRAD_32) == 1, classes

    # (2) the same functional as a sum of 64-image calls: the instantiations depth.npz pins, no 256-row tile
    m2 = _module(sd)

    def chunks():
        for i in range(0, B, 64):
            m2(xc[i:i + 64]).backward(gyc[i:i + 64])

    _, cclasses = _profiled(chunks)
    assert not any(k.endswith(",2,256>") for k in cclasses), cclasses
    for k, p in m2.named_parameters():
        ref = p.grad.cpu().numpy().astype(np.float64)
        err = np.abs(grads[k].cpu().numpy() - ref).max()
        print(f"B = {B}: {k}: one launch vs the sum of 64-image launches: {err / np.abs(ref).max():.2e} of max|g|")
        assert err <= 2e-4 * np.abs(ref).max(), f"{k}: one launch vs the sum of 64-image launches: {err:.3e}, max|g| = {np.abs(ref).max():.3e}"

    # (1) the CPU oracle, fp32 and fp64
    y32, g32 = oe.value_and_grads(oe.depth_backbone, x, sd, gy, chunk=64)
    y64, g64 = oe.value_and_grads(oe.depth_backbone, x, sd, gy, dtype=torch.float64, chunk=64)
    _assert_rows_close(f"B = {B}: y", y, y64, y32)
    for k in sd:
        _assert_close_to_truth(f"B = {B}: {k}", grads[k], g32[k], g64[k])


def test_depth_gradient_of_single_images_at_block_edges():
    """768 images, dy non-zero for six of them only: the first and last image of each 256-image block of the
    position-major data gradient; 511 / 512 are also the last image of the first pass of k_depth_conv1_wgrad and the first of
    its second.  Every other image contributes an exact zero, so the reference is fp64 on those six images alone, and a
    row that lands in the neighbouring image, or an image summed twice or dropped, shows at full size (not at 1 / sqrt(768)
    of the gradient)."""
    B = 768
    sd, x, dy, near = _case(B)
    assert not bool(near[EDGES].any()), near[EDGES]          # (seed chosen on the CPU so that this holds)
    gy = torch.zeros_like(dy)
    gy[EDGES] = dy[EDGES]
    m = _module(sd)
    (y, grads), classes = _profiled(lambda: _forward_backward(m, x.cuda(), gy.cuda()))
    assert classes.get(PM_DGRAD_32) == 1 and classes.get(TALL_FWD_64) == 1, classes
    y32, g32 = oe.value_and_grads(oe.depth_backbone, x[EDGES], sd, dy[EDGES])
    y64, g64 = oe.value_and_grads(oe.depth_backbone, x[EDGES], sd, dy[EDGES], dtype=torch.float64)
    _assert_rows_close("edges: y", y[EDGES], y64, y32)
    for k in sd:
        _assert_close_to_truth(f"edges: {k}", grads[k], g32[k], g64[k])


def test_depth_forward_past_2048_images():
    """2080 images, forward only: k_depth_conv1_fwd runs 2048 workgroups, 32 of which take a second image (2048 .. 2079).
    The forward is per image, so the reference is fp64 on images 0 .. 31 and 2016 .. 2079 (the last images of the first
    pass and all of the second); the forward is continuous, so no tie mask."""
    B = 2080
    sd, x, _ = depth_case(latent=32, batch=B, seed=B)
    m = _module(sd)
    xc = x.cuda()
    with torch.no_grad():
        y, classes = _profiled(lambda: m(xc))
        fresh = m(xc[2048:])
    torch.cuda.synchronize()
    assert classes.get(TALL_FWD_64) == 1, classes
    assert y.shape == (B, 32) and bool(torch.isfinite(y).all())
    rows = list(range(32)) + list(range(2016, B))
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        y64 = oe.depth_backbone(x[rows].double(), sd64)
        y32 = oe.depth_backbone(x[rows], sd)
    _assert_rows_close("B = 2080: y[0:32], y[2016:2080]", y[rows], y64, y32)
    # the second pass against a fresh 32-image call on the same images (one pass, 128-row tiles)
    _assert_rows_close("B = 2080: y[2048:] vs a 32-image call", y[2048:], fresh.cpu())


def test_depth_backward_bit_reproducible_at_scale():
    """Two forward + backward runs at 768 images give the same bits: the 512 x [32][26] partials of conv1's weight gradient
    (two images in some workgroups), the 170 split-K slabs of conv2's and fc1's split-K slabs are summed in a fixed order."""
    sd, x, dy, _ = _case(768)
    m = _module(sd)
    xc, gyc = x.cuda(), dy.cuda()
    y0, g0 = _forward_backward(m, xc, gyc)
    y1, g1 = _forward_backward(m, xc, gyc)
    assert torch.equal(y0, y1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
        assert bool(torch.isfinite(g0[k]).all()), k


def test_direct_ops_refuse_what_the_plan_refuses():
    """make_depth_plan accepts batches that are a multiple of 32 up to 32768 and latents that are a multiple of 4 (>= 4):
    the direct op raises on anything else (the module pads the batch before it calls the op), and the workspace query
    answers 0."""
    from isaacgyminsertion_amd import _lib, ops  # noqa: F401
    L = _lib.lib()
    for b, latent in [(33, 32), (32800, 32), (32, 6)]:
        assert int(L.igi_depth_workspace_bytes(C.byref(_lib.DepthCfg(b, latent)))) == 0, (b, latent)
    assert int(L.igi_depth_workspace_bytes(C.byref(_lib.DepthCfg(32, 4)))) > 0
    sd, _, _ = depth_case(latent=32, batch=1)
    params = torch.cat([v.reshape(-1) for v in sd.values()]).cuda()
    fwd = torch.ops.mi355ppo.depth_backbone_fwd
    y, _ws = fwd(torch.zeros(32, 1, 54, 96, device="cuda"), params, 32)      # the same arguments at an accepted batch
    assert y.shape == (32, 32)
    for b in (33, 32800):
        with pytest.raises(RuntimeError):
            fwd(torch.zeros(b, 1, 54, 96, device="cuda"), params, 32)
    with pytest.raises(RuntimeError):
        fwd(torch.zeros(32, 1, 54, 96, device="cuda"), params, 6)
    sd6 = depth_case(latent=6, batch=1)[0]                                   # ... also with a parameter vector of that size
    with pytest.raises(RuntimeError):
        fwd(torch.zeros(32, 1, 54, 96, device="cuda"), torch.cat([v.reshape(-1) for v in sd6.values()]).cuda(), 6)
    torch.cuda.synchronize()
