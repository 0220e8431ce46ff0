"""The opt-in bf16-input mode of the tactile CNN's convolutions (igi_conv_set_bf16_inputs / ops.conv_bf16_inputs /
offline_train.model.conv_bf16_inputs) on the GPU.

Arithmetic under test: every product term of the three convolutions -- forward, data gradient, weight gradient -- is
float(bf16(a)) * float(bf16(w)), exact in fp32, accumulated in fp32; everything else (bias + ReLU, ReLU', bias-gradient
sums, the soft-argmax, the 128 -> latent Linear, the split-K reduction) is the fp32 path's.

The emulation below is that statement on the CPU: torch convolutions / torch.nn.grad.conv2d_input / conv2d_weight on
operands passed through ``.bfloat16()``.  It takes every layer's INPUT from the device's own fp32 activations (read from
the forward's workspace through igi_tactile_activation_layout) and the ReLU sides from the device's activations too, so
the forward comparison is continuous in the device's result and the backward uses identical masks: no image is masked
out for sitting near a ReLU's zero.

Shapes: 64 images of 32 x 64 (the 128-row row-major tiles of small batches), 32 images of 33 x 47 (odd maps, ragged
tile edges), 768 images of 32 x 64 (the smallest batch of whole 256-image blocks whose convolutions all have >= 512 tall
tiles: tall forward tiles, fused soft-argmax conv3, position-major data gradients and weight gradients; asserted
through the igi_prof_* classes)."""
import ctypes as C
import functools
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
G = np.load(os.path.join(ROOT, "tests", "golden", "encoders.npz"))

KEYS = [("cnn.0.weight", "cnn.0.bias", 2), ("cnn.2.weight", "cnn.2.bias", 1), ("cnn.4.weight", "cnn.4.bias", 1)]
CHANS = (32, 64, 64)
BF16_CLASS = re.compile(r"^gemm_dma_conv_bf16_kernel<")
FP32_CONV_CLASS = re.compile(r"^gemm_dma_kernel<\d+,(true|false),(true|false),[1-6],2,(256|192)>$")   # PC_CONV_* (prof.h)
SHAPES = [(64, 32, 64), (32, 33, 47), (768, 32, 64)]


def _sd():
    tag = "tac32x64"
    return {k[len(tag) + 3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/p/")}


def _bf16r(t):
    """round to nearest even to bf16, back in t's dtype (fp64 values pass through fp32 first: they ARE fp32 values)"""
    return t.float().bfloat16().to(t.dtype)


class _mode:
    """igi_conv_set_bf16_inputs(on) for a block; the previous setting is restored in ``finally``"""

    def __init__(self, on, which="igi_conv_set_bf16_inputs"):
        self.on, self.which = int(on), which

    def __enter__(self):
        from isaacgyminsertion_amd import _lib
        self.fn = getattr(_lib.lib(), self.which)
        self.prev = self.fn(self.on)

    def __exit__(self, *exc):
        self.fn(self.prev)
        return False


def _maps(ws, B, H, W):
    """the three activated maps the forward left in its workspace, as NCHW CPU tensors"""
    from isaacgyminsertion_amd import _lib
    cfg = _lib.TactileCfg(B, H, W, 32)
    off, rows = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    assert _lib.lib().igi_tactile_activation_layout(C.byref(cfg), off, rows) == 0
    hw = [((H - 8) // 2 + 1, (W - 8) // 2 + 1)]
    hw.append((hw[0][0] - 3, hw[0][1] - 3))
    hw.append((hw[1][0] - 2, hw[1][1] - 2))
    out = []
    for l in range(3):
        a = ws[off[l]:off[l] + 4 * rows[l] * CHANS[l]].view(torch.float32).reshape(B, hw[l][0], hw[l][1], CHANS[l])
        out.append(a.permute(0, 3, 1, 2).contiguous().cpu())
    return out


def _split(flat, sd):
    out, o = {}, 0
    for k, v in sd.items():
        out[k] = flat[o:o + v.numel()].reshape(v.shape)
        o += v.numel()
    assert o == flat.numel()
    return out


def _run(x, gy, flat, on, gemm_bf16=False):
    """forward + backward through the two ops under one setting -> (y, grads (flat), workspace, profiler classes)"""
    from isaacgyminsertion_amd import _lib, ops  # noqa: F401
    B, _, H, W = x.shape
    with _mode(on), _mode(gemm_bf16, "igi_gemm_set_bf16_inputs"):
        _lib.prof_enable(True)
        try:
            y, ws = torch.ops.mi355ppo.tactile_cnn_fwd(x, flat, 32)
            g = torch.ops.mi355ppo.tactile_cnn_bwd(gy, flat, ws, H, W)
            torch.cuda.synchronize()
            classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
        finally:
            _lib.prof_enable(False)
    return y, g, ws, classes


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """one device run per shape under the mode (+ the fp32 first map), shared by the tests below and left unchanged"""
    sd = _sd()
    gen = torch.Generator().manual_seed(1000 * B + H)
    x = torch.rand(B, 3, H, W, generator=gen)
    gy = torch.randn(B, 32, generator=gen)
    flat = torch.cat([v.reshape(-1) for v in sd.values()]).cuda()
    y, g, ws, classes = _run(x.cuda(), gy.cuda(), flat, True)
    maps = _maps(ws, B, H, W)
    _y0, _g0, ws0, classes0 = _run(x.cuda(), gy.cuda(), flat, False)
    a1_fp32 = _maps(ws0, B, H, W)[0]
    return dict(sd=sd, x=x, gy=gy, flat=flat, y=y.cpu(), g=_split(g.cpu(), sd), maps=maps, classes=classes,
                classes_fp32=classes0, a1_fp32=a1_fp32)


def _conv_chunked(fn, n, chunk=128):
    return torch.cat([fn(slice(i, min(i + chunk, n))) for i in range(0, n, chunk)])


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_layerwise_forward_is_the_rounded_product(B, H, W):
    """a_l == relu(conv64(bf16r(device a_{l-1}), bf16r(W_l)) + b_l) within the GEMM bound per entry,
    2e-6 * (|bf16r(a)| (*) |bf16r(W)|) + 1e-6 (the abs-sum is evaluated in fp32: a scale, 1e-7 of itself off at most).
    The test discriminates: the UN-rounded fp64 convolution of the same input violates that bound somewhere (rounding
    moves every term by up to 2^-9), and the first map differs from the fp32 path's.  Cannot pass without the mode."""
    c = _case(B, H, W)
    sd, maps = c["sd"], c["maps"]
    inputs = [c["x"], maps[0], maps[1]]
    for l, (kw, kb, stride) in enumerate(KEYS):
        a_in, w = inputs[l], sd[kw]
        ar, wr = _bf16r(a_in), _bf16r(w)
        ref = _conv_chunked(lambda s: F.relu(F.conv2d(ar[s].double(), wr.double(), sd[kb].double(), stride=stride)), B)
        bound = 2e-6 * _conv_chunked(lambda s: F.conv2d(ar[s].abs(), wr.abs(), None, stride=stride), B).double() + 1e-6
        err = (maps[l].double() - ref).abs()
        worst = float((err / bound).max())
        print(f"[{B}x{H}x{W}] conv{l + 1}: max err / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
        assert worst <= 1.0, (l, worst, float(err.max()))
        n = min(B, 32)        # the un-rounded product of the same inputs is NOT what the device computed
        exact = F.relu(F.conv2d(a_in[:n].double(), w.double(), sd[kb].double(), stride=stride))
        viol = float(((maps[l][:n].double() - exact).abs() / bound[:n]).max())
        print(f"[{B}x{H}x{W}] conv{l + 1}: un-rounded fp64 product: max err / bound = {viol:.1f}")
        assert viol > 1.0, (l, viol)
    assert not torch.equal(maps[0], c["a1_fp32"])


def _softargmax_linear(a3, wf, bf):
    from oracle import encoders as oe
    return F.linear(oe.spatial_softargmax(a3, True), wf, bf)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_output_from_the_device_feature_map(B, H, W):
    """y against the fp64 soft-argmax + Linear of the device's a_3 (both fp32 under the mode): 2e-5 abs + 1e-4 rel, the
    tolerance of test_gpu_student_scale.py."""
    c = _case(B, H, W)
    sd = c["sd"]
    y64 = _softargmax_linear(c["maps"][2].double(), sd["cnn.7.weight"].double(), sd["cnn.7.bias"].double())
    np.testing.assert_allclose(c["y"].numpy(), y64.numpy(), atol=2e-5, rtol=1e-4)


def _emulated_backward(c, dtype, chunk=128):
    """The mode's backward in ``dtype`` on the CPU, from the device's activations: the soft-argmax + Linear backward from
    a_3 (autograd), ReLU' from the device's maps, and every convolution operand (dz_l, a_{l-1}, W_l) rounded to bf16
    before each product; bias gradients are plain sums of dz_l.  Chunked over the batch (additive over images)."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    sd = {k: v.to(dtype) for k, v in c["sd"].items()}
    x, gy = c["x"].to(dtype), c["gy"].to(dtype)
    maps = [m.to(dtype) for m in c["maps"]]
    B = x.shape[0]
    g = {k: torch.zeros_like(v) for k, v in sd.items()}
    for i in range(0, B, chunk):
        s = slice(i, min(i + chunk, B))
        a3 = maps[2][s].clone().requires_grad_(True)
        wf, bf = sd["cnn.7.weight"].clone().requires_grad_(True), sd["cnn.7.bias"].clone().requires_grad_(True)
        (_softargmax_linear(a3, wf, bf) * gy[s]).sum().backward()
        g["cnn.7.weight"] += wf.grad
        g["cnn.7.bias"] += bf.grad
        dz = a3.grad * (maps[2][s] > 0).to(dtype)
        ins = [x[s], maps[0][s], maps[1][s]]
        for l in (2, 1, 0):
            kw, kb, stride = KEYS[l]
            dzr, ar, wr = _bf16r(dz), _bf16r(ins[l]), _bf16r(sd[kw])
            g[kw] += conv2d_weight(ar, sd[kw].shape, dzr, stride=stride)
            g[kb] += dz.sum((0, 2, 3))
            if l > 0:
                dz = conv2d_input(ins[l].shape, wr, dzr, stride=stride) * (ins[l] > 0).to(dtype)
    return g


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_gradients_match_the_emulated_backward(B, H, W):
    """All eight parameter tensors: |hip - emulation64| <= max(3e-4 * max|g|, 3 x |emulation32 - emulation64|) per tensor
    -- the bound test_gpu_student_scale.py applies to the fp32 path, with the emulation of THIS arithmetic as the truth."""
    c = _case(B, H, W)
    g64 = _emulated_backward(c, torch.float64)
    g32 = _emulated_backward(c, torch.float32)
    bad = []
    for k in c["sd"]:
        ref = g64[k].numpy()
        scale = np.abs(ref).max()
        err = np.abs(c["g"][k].numpy().astype(np.float64) - ref).max()
        err32 = np.abs(g32[k].numpy().astype(np.float64) - ref).max()
        print(f"[{B}x{H}x{W}] {k}: |hip - emu64| = {err:.3e} ({err / scale:.2e} of max|g|), |emu32 - emu64| = {err32:.3e}")
        if not err <= max(3e-4 * scale, 3.0 * err32):
            bad.append((k, err, err32, scale))
    assert not bad, bad


def test_all_nine_products_ran_as_bf16_conv_classes_at_768():
    """768 images: three tall forward tiles (conv3 with the soft-argmax partials), two position-major data gradients, three
    position-major weight gradients (conv3's on the 192-row tile) -- the classes next to PC_CONV_* in prof.h -- and no
    fp32 convolution class; with the mode off the same nine launches are the fp32 classes."""
    c = _case(768, 32, 64)
    want = {"gemm_dma_conv_bf16_kernel<32,true,true,1,2,256>": 1, "gemm_dma_conv_bf16_kernel<64,true,true,1,2,256>": 1,
            "gemm_dma_conv_bf16_kernel<64,true,true,6,2,256>": 1, "gemm_dma_conv_bf16_kernel<64,true,true,4,2,256>": 1,
            "gemm_dma_conv_bf16_kernel<32,true,true,4,2,256>": 1, "gemm_dma_conv_bf16_kernel<32,false,false,5,2,256>": 1,
            "gemm_dma_conv_bf16_kernel<64,false,false,5,2,256>": 1, "gemm_dma_conv_bf16_kernel<64,false,false,5,2,192>": 1}
    got = {k: v for k, v in c["classes"].items() if BF16_CLASS.match(k)}
    assert got == want, c["classes"]
    assert not [k for k in c["classes"] if FP32_CONV_CLASS.match(k)], c["classes"]
    off = c["classes_fp32"]
    assert not [k for k in off if BF16_CLASS.match(k)], off
    assert sum(v for k, v in off.items() if FP32_CONV_CLASS.match(k)) == 8, off
    # the small shapes: eight bf16 launches as well (row-major 128-row tiles), none booked as fp32
    for shp in SHAPES[:2]:
        cl = _case(*shp)["classes"]
        assert sum(v for k, v in cl.items() if BF16_CLASS.match(k)) == 8, cl
        assert not [k for k in cl if FP32_CONV_CLASS.match(k)], cl


def _module_grads(x, gy, fwd_on, bwd_on):
    from isaacgyminsertion_amd import ops
    from isaacgyminsertion_amd.algo.models.transformer.tactile_cnn import CNNWithSpatialSoftArgmax
    m = CNNWithSpatialSoftArgmax(32)
    m.load_state_dict(_sd())
    m = m.cuda()
    start = ops.conv_bf16_inputs_enabled()
    try:
        ops.conv_bf16_inputs(fwd_on)
        y = m(x)
        ops.conv_bf16_inputs(bwd_on)            # flipped behind the forward's back
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        assert ops.conv_bf16_inputs_enabled() is bool(bwd_on)     # the backward restored what it found
    finally:
        ops.conv_bf16_inputs(start)
    return y.detach(), [p.grad.clone() for p in m.parameters()]


def test_reproducible_and_mode_is_captured_at_forward():
    """Two forward + backward runs under the mode are bit-identical; a switch flipped between forward and backward does
    not reach the backward (the autograd formula re-establishes the forward's setting): on/off == on/on, off/on == off/off."""
    gen = torch.Generator().manual_seed(5)
    x, gy = torch.rand(64, 3, 32, 64, generator=gen).cuda(), torch.randn(64, 32, generator=gen).cuda()
    y_on, g_on = _module_grads(x, gy, True, True)
    y_on2, g_on2 = _module_grads(x, gy, True, True)
    assert torch.equal(y_on, y_on2) and all(torch.equal(a, b) for a, b in zip(g_on, g_on2))
    y_off, g_off = _module_grads(x, gy, False, False)
    assert not torch.equal(y_on, y_off) and not torch.equal(g_on[0], g_off[0])
    y_a, g_a = _module_grads(x, gy, True, False)
    assert torch.equal(y_a, y_on) and all(torch.equal(a, b) for a, b in zip(g_a, g_on))
    y_b, g_b = _module_grads(x, gy, False, True)
    assert torch.equal(y_b, y_off) and all(torch.equal(a, b) for a, b in zip(g_b, g_off))
    # the large tiles reproduce too (two runs of the ops at 768 images)
    c = _case(768, 32, 64)
    y2, g2, _ws, _cl = _run(c["x"].cuda(), c["gy"].cuda(), c["flat"], True)
    assert torch.equal(y2.cpu(), c["y"]) and torch.equal(g2.cpu(), torch.cat([v.reshape(-1) for v in c["g"].values()]))


def _others():
    """results of everything the conv switch must not touch, under the setting in force"""
    from isaacgyminsertion_amd.hip_token_encoder import HipTransformerEncoder
    from isaacgyminsertion_amd.teacher_native import TeacherEngine
    from oracle import synth
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    out = {}
    pc, pp = torch.randn(9, 400, 3, device=dev, generator=g) * 0.5, torch.randn(16896, device=dev, generator=g) * 0.2
    out["pointnet_y"], out["pointnet_idx"] = torch.ops.mi355ppo.pointnet_max_fwd(pc, pp)
    x, w, b = (torch.randn(*s, device=dev, generator=g) for s in ((512, 256), (128, 256), (128,)))
    out["linear"] = torch.ops.mi355ppo.linear(x, w * 0.05, b, 1)
    torch.manual_seed(0)
    layer = torch.nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=128, activation="gelu",
                                             batch_first=True, norm_first=True, dropout=0.0)
    enc = HipTransformerEncoder(layer, 2).to(dev).eval()
    with torch.no_grad():
        out["token"] = enc(torch.randn(64, 3, 32, device=dev, generator=g))
    N, T, E = 64, 8, 2
    units, priv_units = [64, 48, 32], [48, 32, 8]
    init, ro, perm = synth.teacher_problem(N, T, units, priv_units, seed=9, done_p=0.1)
    eng = TeacherEngine(N, T, E, units=units, priv_units=priv_units, perm=perm)
    eng.load_params(init)
    obs, priv = torch.randn(50, 15, device=dev, generator=g), torch.randn(50, 64, device=dev, generator=g)
    out["infer_mu"], out["infer_v"] = eng.infer(obs, priv)[:2]          # torch.ops.mi355ppo.actor_critic_infer
    eng.prepare(ro)
    out["teacher_stats"] = eng.update().clone()
    out["teacher_params"] = eng.packed().clone()
    torch.cuda.synchronize()
    return out


def test_isolation_from_everything_else_and_from_the_gemm_switch():
    """With the conv switch on, PointNet, ``linear``, the token encoder, ``actor_critic_infer`` and a small teacher update
    are bit-identical to switch-off.  With only igi_gemm_set_bf16_inputs(1) on, the tactile forward and gradients are
    bit-identical to the fp32 run: that switch keeps excluding the im2col products."""
    with _mode(False):
        ref = _others()
    with _mode(True):
        got = _others()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    c = _case(64, 32, 64)
    x, gy = c["x"].cuda(), c["gy"].cuda()
    y0, g0, _ws, cl0 = _run(x, gy, c["flat"], False)
    y1, g1, _ws, cl1 = _run(x, gy, c["flat"], False, gemm_bf16=True)
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    assert not [k for k in cl1 if BF16_CLASS.match(k)], cl1


_TRAINER = r"""
import json, sys, torch
sys.path.insert(0, %(root)r)
from isaacgyminsertion_amd import _lib
from isaacgyminsertion_amd.algo.ext_adapt.ext_adapt import ExtrinsicAdapt
from isaacgyminsertion_amd.envs.synthetic import SyntheticInsertionEnv
from isaacgyminsertion_amd.utils.config import default_config

def run(key):
    dev = "cuda:0"
    cfg = default_config(num_envs=8, horizon_length=4, rl_device=dev, mini_epochs=4, obs_info=True, tactile_info=True,
                         pcl_info=False, img_info=False, seg_info=False, num_points=8)
    if key is None:
        del cfg.offline_train.model["conv_bf16_inputs"]
    else:
        cfg.offline_train.model.conv_bf16_inputs = key
    env = SyntheticInsertionEnv(8, device=dev, tactile_hw=(32, 64), pcl_points=0, img_hw=None)
    torch.manual_seed(0)
    agent = ExtrinsicAdapt(env, None, cfg)
    g = torch.Generator(device=dev).manual_seed(0)
    st = agent.storage.storage_dict
    st["n_tactile"].uniform_(0, 1, generator=g)
    st["n_student_obs"].normal_(generator=g)
    st["teacher_actions"].uniform_(-1.2, 1.2, generator=g)
    for m in agent.student.model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    agent.storage.prepare_training()
    agent.set_student_train()
    before = _lib.lib().igi_conv_set_bf16_inputs(-1)
    _lib.prof_enable(True)
    losses, _ = agent.update()
    torch.cuda.synchronize()
    classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    _lib.prof_enable(False)
    return {"losses": [float(l) for l in losses], "classes": classes, "switch_before": before,
            "switch_after": _lib.lib().igi_conv_set_bf16_inputs(-1)}

print(json.dumps({"on": run(True), "absent": run(None)}))
"""


def test_trainer_reads_the_config_key():
    """ExtrinsicAdapt (tactile + lin, 8 envs x 4 steps, 4 mini-epochs) in a child process with
    offline_train.model.conv_bf16_inputs=True: update() runs bf16 convolution classes and no fp32 one, the loss falls
    over the update (mean of the last mini-epoch below the first's), and the process switch is left as it was; the same
    run without the key shows no bf16 class."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("IGI_CONV_BF16", None)
    r = subprocess.run([sys.executable, "-c", _TRAINER % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    on, absent = out["on"], out["absent"]
    assert sum(v for k, v in on["classes"].items() if BF16_CLASS.match(k)) >= 8 * len(on["losses"]), on["classes"]
    assert not [k for k in on["classes"] if FP32_CONV_CLASS.match(k)], on["classes"]
    assert on["switch_before"] == 0 and on["switch_after"] == 0
    n = len(on["losses"]) // 4
    first, last = np.mean(on["losses"][:n]), np.mean(on["losses"][-n:])
    print(f"loss: first mini-epoch {first:.5f}, last {last:.5f}")
    assert np.isfinite(on["losses"]).all() and last < first, on["losses"]
    assert not [k for k in absent["classes"] if BF16_CLASS.match(k)], absent["classes"]
    assert [k for k in absent["classes"] if FP32_CONV_CLASS.match(k)], absent["classes"]
