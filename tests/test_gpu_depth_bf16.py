"""The opt-in bf16-input mode of the depth backbone (igi_depth_set_bf16_inputs / ops.depth_bf16_inputs /
offline_train.model.depth_bf16_inputs) on the GPU.

Arithmetic under test: every product term of conv2 (forward, data gradient, weight gradient) and of the 64768 -> 128
Linear "fc1" (split-K forward, data gradient with its ELU' epilogue, weight gradient) is float(bf16(a)) * float(bf16(b)),
exact in fp32, accumulated in fp32.  conv1 + max-pool + ELU with its arg-max bytes, conv1's weight gradient, the
128 -> latent Linear, biases, bias-gradient sums, ELU / ELU' and the split-K reductions are the fp32 path's, bit for bit.

tests/depth_bf16_ref.py is that statement on the CPU.  Every check takes a layer's INPUT from the device's own fp32
activations (igi_depth_activation_layout), ELU' from the device's maps and the pool routing from the device's arg-max
bytes, so the comparisons are continuous in the device's result: no image is masked out, the share left out is 0.

Shapes: depth_case(32, B, seed=B) at B = 64 (128-row im2col tiles), 160 (256-row conv2 forward tile, row-major tall data
gradient) and 768 (position-major data gradient, 170-way weight-gradient split): the smallest batches at which each
dispatch regime of tests/test_gpu_depth_scale.py is live, asserted through the igi_prof_* classes."""
import ctypes as C
import functools
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import depth_bf16_ref as ref  # noqa: E402
from depth_bf16_ref import B1, B2, BF1, BF2, W1, W2, WF1, WF2, bf16r  # noqa: E402,F401
from make_golden_depth import depth_case  # noqa: E402  (seeded inputs only; the reference is not imported)

SHAPES = [64, 160, 768]
# profiler classes (csrc/prof.h).  fp32: the six products by batch regime, as tests/test_gpu_depth_scale.py lists them
FC1_FP32 = ["gemm_dma_kernel<128,true,true>", "gemm_dma_kernel<128,true,false>", "gemm_dma_kernel<128,false,false>"]
FC1_BF16 = ["gemm_dma_bf16_kernel<true,true>", "gemm_dma_bf16_kernel<true,false>", "gemm_dma_bf16_kernel<false,false>"]
ROW64_FP32, ROW64_BF16 = "gemm_dma_kernel<64,true,true>", "gemm_dma_conv_bf16_kernel<64,true,true,1,3,128>"
WG_FP32, WG_BF16 = "gemm_dma_kernel<64,false,false>", "gemm_dma_conv_bf16_kernel<64,false,false,5,3,128>"
TALL = "1,2,256>"       # conv2 forward 64-wide / data gradient 32-wide, row-major 256-row tiles
PM = "4,2,256>"         # data gradient, position-major
# regime -> (fp32 class, bf16 class) of conv2's forward and data gradient
CONV_FWD = {64: (ROW64_FP32, ROW64_BF16),
            160: ("gemm_dma_kernel<64,true,true," + TALL, "gemm_dma_conv_bf16_kernel<64,true,true," + TALL),
            768: ("gemm_dma_kernel<64,true,true," + TALL, "gemm_dma_conv_bf16_kernel<64,true,true," + TALL)}
CONV_DGRAD = {64: (ROW64_FP32, ROW64_BF16),
              160: ("gemm_dma_kernel<32,true,true," + TALL, "gemm_dma_conv_bf16_kernel<32,true,true," + TALL),
              768: ("gemm_dma_kernel<32,true,true," + PM, "gemm_dma_conv_bf16_kernel<32,true,true," + PM)}
BF16_CLASS = re.compile(r"^gemm_dma_(conv_)?bf16_kernel<")
# what the six products are booked as with the mode off; "<64,true,true>" is shared with the 128 -> latent Linear (fp32 always)
FP32_SIX = re.compile(r"^gemm_dma_kernel<(128,(true,true|true,false|false,false)|64,false,false|\d+,true,true,[14],2,256)>$")


class _mode:
    """one of the three bf16-input switches for a block; the previous setting is restored in ``finally``"""

    def __init__(self, on, which="igi_depth_set_bf16_inputs"):
        self.on, self.which = int(on), which

    def __enter__(self):
        from isaacgyminsertion_amd import _lib
        self.fn = getattr(_lib.lib(), self.which)
        self.prev = self.fn(self.on)

    def __exit__(self, *exc):
        self.fn(self.prev)
        return False


def _maps(ws, B):
    """(a1, arg-max bytes, a2, h3) the forward left in its workspace: NCHW CPU tensors, h3 (B, 128)"""
    from isaacgyminsertion_amd import _lib
    off, rows = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    assert _lib.lib().igi_depth_activation_layout(C.byref(_lib.DepthCfg(B, 32)), off, rows) == 0
    assert list(rows) == [B * 1150, B * 1012, B]
    n1 = rows[0] * 32
    a1 = ws[off[0]:off[0] + 4 * n1].view(torch.float32).reshape(B, 25, 46, 32).permute(0, 3, 1, 2).contiguous().cpu()
    idx = ws[off[0] + 4 * n1:off[0] + 5 * n1].reshape(B, 25, 46, 32).permute(0, 3, 1, 2).contiguous().cpu()
    a2 = ws[off[1]:off[1] + 4 * rows[1] * 64].view(torch.float32).reshape(B, 23, 44, 64).permute(0, 3, 1, 2).contiguous().cpu()
    h3 = ws[off[2]:off[2] + 4 * B * 128].view(torch.float32).reshape(B, 128).cpu()
    return a1, idx, a2, h3


def _split(flat, sd):
    out, o = {}, 0
    for k, v in sd.items():
        out[k] = flat[o:o + v.numel()].reshape(v.shape)
        o += v.numel()
    assert o == flat.numel()
    return out


def _run(x, gy, flat, on, gemm_bf16=False, conv_bf16=False):
    """forward + backward through the two ops under one setting -> (y, grads (flat), workspace, profiler classes)"""
    from isaacgyminsertion_amd import _lib, ops  # noqa: F401
    with _mode(on), _mode(gemm_bf16, "igi_gemm_set_bf16_inputs"), _mode(conv_bf16, "igi_conv_set_bf16_inputs"):
        _lib.prof_enable(True)
        try:
            y, ws = torch.ops.mi355ppo.depth_backbone_fwd(x, flat, 32)
            g = torch.ops.mi355ppo.depth_backbone_bwd(x, gy, flat, ws)
            torch.cuda.synchronize()
            classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
        finally:
            _lib.prof_enable(False)
    return y, g, ws, classes


@functools.lru_cache(maxsize=None)
def _case(B):
    """one device run per shape under the mode and one with it off, shared by the tests below and left unchanged"""
    sd, x, gy = depth_case(latent=32, batch=B, seed=B)
    flat = torch.cat([v.reshape(-1) for v in sd.values()]).cuda()
    y, g, ws, classes = _run(x.cuda(), gy.cuda(), flat, True)
    a1, idx, a2, h3 = _maps(ws, B)
    y0, g0, ws0, classes0 = _run(x.cuda(), gy.cuda(), flat, False)
    a1_0, idx_0, a2_0, _h3_0 = _maps(ws0, B)
    del ws, ws0
    return dict(sd=sd, x=x, gy=gy, flat=flat, y=y.cpu(), g=_split(g.cpu(), sd), a1=a1, idx=idx, a2=a2, h3=h3,
                classes=classes, y_fp32=y0.cpu(), g_fp32=g0.cpu(), a1_fp32=a1_0, idx_fp32=idx_0, a2_fp32=a2_0,
                classes_fp32=classes0)


def _chunked(fn, n, chunk=64):
    return torch.cat([fn(slice(i, min(i + chunk, n))) for i in range(0, n, chunk)])


@pytest.mark.parametrize("B", SHAPES)
def test_conv1_is_untouched(B):
    """a1 and the pool's arg-max bytes under the mode are the fp32 path's, bit for bit: conv1 stays fp32 and the mode
    changes no pool decision."""
    c = _case(B)
    assert torch.equal(c["a1"], c["a1_fp32"]) and torch.equal(c["idx"], c["idx_fp32"])
    assert int(c["idx"].max()) <= 3


@pytest.mark.parametrize("B", SHAPES)
def test_conv2_forward_is_the_rounded_product(B):
    """a2 == elu(conv64(bf16r(device a1), bf16r(W2)) + b2) per entry within the GEMM bound of tests/test_gpu_tactile_bf16.py,
    2e-6 * (|bf16r(a)| (*) |bf16r(W)|) + 1e-6 (the abs-sum is evaluated in fp32: a scale).  The UN-rounded fp64 product of
    the same inputs violates that bound somewhere, and a2 differs from the fp32 path's: cannot pass without the mode."""
    c = _case(B)
    sd, a1, a2 = c["sd"], c["a1"], c["a2"]
    ar, wr = bf16r(a1), bf16r(sd[W2])
    want = _chunked(lambda s: F.elu(F.conv2d(ar[s].double(), wr.double(), sd[B2].double())), B)
    bound = 2e-6 * _chunked(lambda s: F.conv2d(ar[s].abs(), wr.abs()), B).double() + 1e-6
    err = (a2.double() - want).abs()
    worst = float((err / bound).max())
    print(f"[{B}] conv2: max err / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
    assert worst <= 1.0, (worst, float(err.max()))
    n = min(B, 32)
    exact = F.elu(F.conv2d(a1[:n].double(), sd[W2].double(), sd[B2].double()))
    viol = float(((a2[:n].double() - exact).abs() / bound[:n]).max())
    print(f"[{B}] conv2: un-rounded fp64 product: max err / bound = {viol:.1f}")
    assert viol > 1.0, viol
    assert not torch.equal(a2, c["a2_fp32"])


@pytest.mark.parametrize("B", SHAPES)
def test_fc1_forward_is_the_rounded_product(B):
    """h3 == elu(bf16r(device a2) . bf16r(Wfc1)^T + b) per entry within the same bound, 2e-6 * abs-sum + 1e-6, at
    K = 64768 (the abs-sum in fp64 here: 64768 fp32 additions would move the scale itself); the un-rounded fp64 product
    violates it.  The factor 2e-6 held as it stands: no measured factor had to be granted."""
    c = _case(B)
    sd = c["sd"]
    ar, wr = bf16r(c["a2"].flatten(1)).double(), bf16r(sd[WF1]).double()
    want = F.elu(ar @ wr.t() + sd[BF1].double())
    bound = 2e-6 * (ar.abs() @ wr.abs().t()) + 1e-6
    err = (c["h3"].double() - want).abs()
    worst = float((err / bound).max())
    print(f"[{B}] fc1: max err / bound = {worst:.3f}, max err = {float(err.max()):.3e}, "
          f"max err / abs-sum = {float((err / (bound - 1e-6) * 2e-6).max()):.3e}")
    assert worst <= 1.0, (worst, float(err.max()))
    exact = F.elu(c["a2"].flatten(1).double() @ sd[WF1].double().t() + sd[BF1].double())
    viol = float(((c["h3"].double() - exact).abs() / bound).max())
    print(f"[{B}] fc1: un-rounded fp64 product: max err / bound = {viol:.1f}")
    assert viol > 1.0, viol


@pytest.mark.parametrize("B", SHAPES)
def test_output_from_the_device_h3(B):
    """y against the fp64 Linear(128 -> latent) of the device's h3 (fp32 under the mode too): 2e-5 abs + 1e-4 rel"""
    c = _case(B)
    sd = c["sd"]
    y64 = F.linear(c["h3"].double(), sd[WF2].double(), sd[BF2].double())
    np.testing.assert_allclose(c["y"].numpy(), y64.numpy(), atol=2e-5, rtol=1e-4)
    assert not torch.equal(c["y"], c["y_fp32"])


def _emulated_backward(c, dtype):
    sd = {k: v.to(dtype) for k, v in c["sd"].items()}
    return ref.backward(c["x"].to(dtype), c["gy"].to(dtype), sd, c["a1"].to(dtype), c["idx"], c["a2"].to(dtype),
                        c["h3"].to(dtype))


@pytest.mark.parametrize("B", SHAPES)
def test_gradients_match_the_emulated_backward(B):
    """All eight parameter tensors against tests/depth_bf16_ref.py:backward from the device's activations:
    |hip - emulation64| <= max(3e-4 * max|g|, 3 x |emulation32 - emulation64|) per tensor.  No image is masked out."""
    c = _case(B)
    g64 = _emulated_backward(c, torch.float64)
    g32 = _emulated_backward(c, torch.float32)
    bad = []
    for k in c["sd"]:
        want = g64[k].numpy()
        scale = np.abs(want).max()
        err = np.abs(c["g"][k].numpy().astype(np.float64) - want).max()
        err32 = np.abs(g32[k].numpy().astype(np.float64) - want).max()
        print(f"[{B}] {k}: |hip - emu64| = {err:.3e} ({err / scale:.2e} of max|g|), |emu32 - emu64| = {err32:.3e}")
        if not err <= max(3e-4 * scale, 3.0 * err32):
            bad.append((k, err, err32, scale))
    assert not bad, bad
    assert not torch.equal(torch.cat([v.reshape(-1) for v in c["g"].values()]), c["g_fp32"])


@pytest.mark.parametrize("B", SHAPES)
def test_the_six_products_ran_as_bf16_classes(B):
    """Mode off: the gemm_dma_kernel classes are exactly today's (tests/test_gpu_depth_scale.py lists them).  Mode on: the
    six products moved to the bf16 twin of the SAME tile, one launch each, none is booked under an fp32 class, and
    every other class of the run is unchanged."""
    c = _case(B)
    on, off = c["classes"], c["classes_fp32"]
    print(f"[{B}] off: {off}\n[{B}] on: {on}")
    fwd, dgrad = CONV_FWD[B], CONV_DGRAD[B]
    today = {k: 1 for k in FC1_FP32}
    today[WG_FP32] = 1
    today[ROW64_FP32] = 1                      # the 128 -> latent Linear's forward
    today[fwd[0]] = today.get(fwd[0], 0) + 1
    today[dgrad[0]] = today.get(dgrad[0], 0) + 1
    assert {k: v for k, v in off.items() if k.startswith("gemm_dma_kernel<")} == today, off
    assert not [k for k in off if BF16_CLASS.match(k)], off
    want = dict(off)
    for a, b in list(zip(FC1_FP32, FC1_BF16)) + [(WG_FP32, WG_BF16), fwd, dgrad]:
        want[a] -= 1
        want[b] = want.get(b, 0) + 1
    want = {k: v for k, v in want.items() if v}
    assert on == want, (on, want)
    assert sum(v for k, v in on.items() if BF16_CLASS.match(k)) == 6
    assert not [k for k in on if FP32_SIX.match(k)], on


def _module_grads(sd, x, gy, fwd_on, bwd_on):
    from isaacgyminsertion_amd import ops
    from isaacgyminsertion_amd.algo.models.transformer.depth_backbone import DepthOnlyFCBackbone54x96
    m = DepthOnlyFCBackbone54x96(latent_dim=32)
    m.load_state_dict(sd)
    m = m.cuda()
    start = ops.depth_bf16_inputs_enabled()
    try:
        ops.depth_bf16_inputs(fwd_on)
        y = m(x)
        ops.depth_bf16_inputs(bwd_on)           # flipped behind the forward's back
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        assert ops.depth_bf16_inputs_enabled() is bool(bwd_on)    # the backward restored what it found
    finally:
        ops.depth_bf16_inputs(start)
    return y.detach(), [p.grad.clone() for p in m.parameters()]


def test_reproducible_and_mode_is_captured_at_forward():
    """Two forward + backward runs under the mode are bit-identical (also at 768 images); a switch flipped between forward
    and backward does not reach the backward: on/off == on/on, off/on == off/off."""
    c = _case(64)
    x, gy = c["x"].cuda(), c["gy"].cuda()
    y_on, g_on = _module_grads(c["sd"], x, gy, True, True)
    y_on2, g_on2 = _module_grads(c["sd"], x, gy, True, True)
    assert torch.equal(y_on, y_on2) and all(torch.equal(a, b) for a, b in zip(g_on, g_on2))
    y_off, g_off = _module_grads(c["sd"], x, gy, False, False)
    assert not torch.equal(y_on, y_off) and not torch.equal(g_on[2], g_off[2])
    assert torch.equal(y_on.cpu(), c["y"]) and torch.equal(y_off.cpu(), c["y_fp32"])          # the module is the ops
    y_a, g_a = _module_grads(c["sd"], x, gy, True, False)
    assert torch.equal(y_a, y_on) and all(torch.equal(a, b) for a, b in zip(g_a, g_on))
    y_b, g_b = _module_grads(c["sd"], x, gy, False, True)
    assert torch.equal(y_b, y_off) and all(torch.equal(a, b) for a, b in zip(g_b, g_off))
    c = _case(768)
    y2, g2, _ws, _cl = _run(c["x"].cuda(), c["gy"].cuda(), c["flat"], True)
    assert torch.equal(y2.cpu(), c["y"]) and torch.equal(g2.cpu(), torch.cat([v.reshape(-1) for v in c["g"].values()]))


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# sha256 over (y, grads) of depth_case(32, 64, seed=64) under igi_gemm_set_bf16_inputs(1), recorded once from a build of the
# commit before this mode existed, in a child process of its own (the digest function above, the ops of _run)
PARENT_GEMM_BF16_DIGEST = "2526c4d5bf7636b34042bac81352fa0daecb84c9a4bb25e6d7a1e5c5d505812b"


def test_isolation_both_ways():
    """Depth switch on: the tactile CNN, PointNet, ``linear``, the token encoder, ``actor_critic_infer`` and a small
    teacher update are bit-identical to switch off.  Only igi_conv_set_bf16_inputs(1) on: the depth backbone is bit-identical
    to all-off.  Depth switch off under igi_gemm_set_bf16_inputs(1): what the build before this mode gave under that
    switch (the recorded digest), and not the depth mode's result."""
    import test_gpu_tactile_bf16 as tb

    def others():
        out = tb._others()
        sd = tb._sd()
        gen = torch.Generator().manual_seed(7)
        x, gy = torch.rand(32, 3, 32, 64, generator=gen).cuda(), torch.randn(32, 32, generator=gen).cuda()
        flat = torch.cat([v.reshape(-1) for v in sd.values()]).cuda()
        out["tactile_y"], ws = torch.ops.mi355ppo.tactile_cnn_fwd(x, flat, 32)
        out["tactile_g"] = torch.ops.mi355ppo.tactile_cnn_bwd(gy, flat, ws, 32, 64)
        torch.cuda.synchronize()
        return out

    with _mode(False):
        want = others()
    with _mode(True):
        got = others()
    for k in want:
        assert torch.equal(want[k], got[k]), k
    c = _case(64)
    x, gy = c["x"].cuda(), c["gy"].cuda()
    y1, g1, _ws, cl1 = _run(x, gy, c["flat"], False, conv_bf16=True)
    assert torch.equal(y1.cpu(), c["y_fp32"]) and torch.equal(g1.cpu(), c["g_fp32"])
    assert not [k for k in cl1 if BF16_CLASS.match(k)], cl1
    y2, g2, _ws, cl2 = _run(x, gy, c["flat"], False, gemm_bf16=True)
    assert not [k for k in cl2 if BF16_CLASS.match(k)], cl2
    assert not torch.equal(y2.cpu(), c["y"]) and not torch.equal(y2.cpu(), c["y_fp32"])
    assert _digest(y2, g2) == PARENT_GEMM_BF16_DIGEST


_TRAINER = r"""
import json, sys, torch
sys.path.insert(0, %(root)r)
from isaacgyminsertion_amd import _lib
from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
from isaacgyminsertion_amd.utils.config import default_config

def run(key):
    dev = "cuda:0"
    cfg = default_config(num_envs=8, horizon_length=4, rl_device=dev, mini_epochs=4, obs_info=True, tactile_info=False,
                         pcl_info=False, img_info=True, seg_info=True, num_points=8)
    assert "depth_bf16_inputs" not in cfg.offline_train.model
    if key is not None:
        cfg.offline_train.model.depth_bf16_inputs = key
    env = SyntheticInsertionEnv(8, device=dev, tactile_hw=None, pcl_points=0, img_hw=(54, 96))
    torch.manual_seed(0)
    agent = ExtrinsicAdapt(env, None, cfg)
    g = torch.Generator(device=dev).manual_seed(0)
    st = agent.storage.storage_dict
    st["n_img"].uniform_(0, 1, generator=g)
    st["n_seg"].uniform_(0, 1, generator=g)
    st["n_student_obs"].normal_(generator=g)
    st["teacher_actions"].uniform_(-1.2, 1.2, generator=g)
    for m in agent.student.model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    agent.storage.prepare_training()
    agent.set_student_train()
    before = _lib.lib().igi_depth_set_bf16_inputs(-1)
    _lib.prof_enable(True)
    losses, _ = agent.update()
    torch.cuda.synchronize()
    classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    _lib.prof_enable(False)
    return {"losses": [float(l) for l in losses], "classes": classes, "switch_before": before,
            "switch_after": _lib.lib().igi_depth_set_bf16_inputs(-1)}

print(json.dumps({"on": run(True), "absent": run(None)}))
"""


def test_trainer_reads_the_config_key():
    """ExtrinsicAdapt (img_info + seg_info + obs_info, 8 envs x 4 steps, 4 mini-epochs, dropout 0) in a child process with
    offline_train.model.depth_bf16_inputs=True: update() books the bf16 depth classes -- six per backbone and step -- and
    no fp32 conv2 / fc1 class, the loss falls from the first mini-epoch to the last, and the process switch is left as
    found; the same run with the key absent books no bf16 class."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("IGI_DEPTH_BF16", "IGI_CONV_BF16", "IGI_GEMM_BF16"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _TRAINER % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    on, absent = out["on"], out["absent"]
    print(on["classes"], on["losses"])
    assert sum(v for k, v in on["classes"].items() if BF16_CLASS.match(k)) >= 2 * 6 * len(on["losses"]), on["classes"]
    assert not [k for k in on["classes"] if FP32_SIX.match(k)], on["classes"]
    assert on["switch_before"] == 0 and on["switch_after"] == 0
    n = len(on["losses"]) // 4
    first, last = np.mean(on["losses"][:n]), np.mean(on["losses"][-n:])
    print(f"loss: first mini-epoch {first:.5f}, last {last:.5f}")
    assert np.isfinite(on["losses"]).all() and last < first, on["losses"]
    assert not [k for k in absent["classes"] if BF16_CLASS.match(k)], absent["classes"]
    # (at 32 padded images per step conv2's forward / data gradient share "<64,true,true>" with the 128 -> latent Linear, and
    #  fc1's one-k-tile weight gradient shares "<64,false,false>" with conv2's: four countable launches per backbone)
    assert sum(v for k, v in absent["classes"].items() if FP32_SIX.match(k)) >= 2 * 4 * len(absent["losses"]), absent["classes"]


def test_runner_offline_batch_and_predict():
    """Runner with offline_train.model.depth_bf16_inputs=True on one offline batch (camera + segmentation + lin): the
    forward / backward of both backbones run the bf16 classes, an optimizer step leaves finite parameters, predict()
    afterwards runs the bf16 forward classes too, and the process switch is off outside the Runner's calls."""
    from isaacgyminsertion_amd import _lib, ops
    from isaacgyminsertion_amd.algo.models.transformer.runner import Runner
    from isaacgyminsertion_amd.utils.config import default_config, merge
    cfg = default_config(num_envs=8, horizon_length=4, rl_device="cuda:0")
    cfg = merge(cfg, {"offline_train": {"model": {"linear": {"input_size": 18}, "use_tactile": False, "use_img": True,
                                                  "use_seg": True, "depth_bf16_inputs": True}}})
    torch.manual_seed(0)
    r = Runner(cfg, agent=None)
    assert r.depth_bf16_inputs is True and r.conv_bf16_inputs is False
    r.optimizer = r._make_optimizer(1e-3)
    r.loss_fn_mean = torch.nn.MSELoss(reduction='mean')
    gen = torch.Generator().manual_seed(1)
    n = 16
    img, seg = torch.rand(n, 1, 1, 54, 96, generator=gen), torch.rand(n, 1, 1, 54, 96, generator=gen)
    so, act = torch.randn(n, 1, 18, generator=gen), torch.rand(n, 1, 6, generator=gen) * 2 - 1
    z = torch.zeros(n, 1)
    batch = (z, img, seg, so, z, torch.zeros(n, 1, 15), torch.zeros(n, 1, 8), act)
    assert ops.depth_bf16_inputs_enabled() is False
    _lib.prof_enable(True)
    try:
        r.model.train()
        loss = r._forward_loss(batch, clamp=False)[0]
        assert ops.depth_bf16_inputs_enabled() is False
        r.optimizer.zero_grad()
        loss.backward()
        r.optimizer.step()
        torch.cuda.synchronize()
        train_classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    assert sum(v for k, v in train_classes.items() if BF16_CLASS.match(k)) == 12, train_classes
    assert not [k for k in train_classes if FP32_SIX.match(k)], train_classes
    assert np.isfinite(float(loss.detach())) and all(bool(torch.isfinite(p).all()) for p in r.model.parameters())
    _lib.prof_enable(True)
    try:
        out, _ = r.predict({"img": img.reshape(n, 1, -1), "seg": seg.reshape(n, 1, -1), "student_obs": so})
        torch.cuda.synchronize()
        pred_classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
    assert out.shape == (n, 6) and bool(torch.isfinite(out).all())
    assert sum(v for k, v in pred_classes.items() if BF16_CLASS.match(k)) == 4, pred_classes
    assert ops.depth_bf16_inputs_enabled() is False


def test_opcheck_under_the_mode():
    """torch.library.opcheck of the two depth ops with the switch on (the selection of tests/test_gpu_ops.py)"""
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    sd, x, _gy = depth_case(latent=32, batch=32, seed=3)
    x = x.cuda()
    p = torch.cat([v.reshape(-1) for v in sd.values()]).cuda().requires_grad_()
    o = torch.ops.mi355ppo
    with _mode(True):
        torch.library.opcheck(o.depth_backbone_fwd, (x, p, 32), test_utils=tests)
        _y, ws = o.depth_backbone_fwd(x, p.detach(), 32)
        torch.library.opcheck(o.depth_backbone_bwd, (x, torch.randn(32, 32, device="cuda"), p.detach(), ws),
                              test_utils=tests + ("test_aot_dispatch_static",))
