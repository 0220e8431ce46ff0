"""The opt-in split-bf16 mode of the tactile CNN's convolutions (igi_conv_set_bf16x3 / ops.conv_bf16x3 /
offline_train.model.conv_bf16x3) on the GPU.

Arithmetic under test (tests/conv_x3_ref.py states it on the CPU): every operand of the three convolutions -- forward,
data gradient, weight gradient -- is split exactly into three bf16 planes where the MFMA operands are formed, every
product term is the sum of six exact plane products accumulated in fp32 on the bf16 matrix pipe; everything else (bias +
ReLU, ReLU', bias-gradient sums, the soft-argmax, the 128 -> latent Linear, the split-K reduction) is the fp32 path's.
The claim is fp32-GRADE accuracy, so every check here is the one the fp32 path is held to, against UN-rounded float64 --
and each is shown to reject the one-plane mode (igi_conv_set_bf16_inputs), so the two cannot be confused.

As in tests/test_gpu_tactile_bf16.py, every layer's INPUT and the ReLU sides are read from the device's own workspace
(igi_tactile_activation_layout): no image is masked out for sitting near a ReLU's zero.

Shapes (those of the bf16 test): 64 images of 32 x 64 (the 128-row tiles of small batches), 32 images of 33 x 47 (odd
maps, ragged tile edges), 768 images of 32 x 64 (tall forward tiles, fused soft-argmax conv3, position-major data and
weight gradients, the 192-row tile; asserted through the igi_prof_* classes)."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_x3_ref import bf16r  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "encoders.npz"))

KEYS = [("cnn.0.weight", "cnn.0.bias", 2), ("cnn.2.weight", "cnn.2.bias", 1), ("cnn.4.weight", "cnn.4.bias", 1)]
CHANS = (32, 64, 64)
X3_CLASS = re.compile(r"^gemm_dma_conv_x3_kernel<")
BF16_CLASS = re.compile(r"^gemm_dma_conv_bf16_kernel<")
FP32_CONV_CLASS = re.compile(r"^gemm_dma_kernel<\d+,(true|false),(true|false),[1-6],2,(256|192)>$")   # PC_CONV_* (prof.h)
SHAPES = [(64, 32, 64), (32, 33, 47), (768, 32, 64)]
SWITCHES = ("igi_conv_set_bf16x3", "igi_conv_set_bf16_inputs", "igi_gemm_set_bf16_inputs", "igi_gemm_set_bf16x3")


def _sd():
    tag = "tac32x64"
    return {k[len(tag) + 3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith(f"{tag}/p/")}


class _mode:
    """process switches for a block, by entry-point name; the previous settings are restored on the way out"""

    def __init__(self, **on):
        self.on = on

    def __enter__(self):
        from isaacgyminsertion_amd import _lib
        self.prev = {k: getattr(_lib.lib(), k)(int(v)) for k, v in self.on.items()}

    def __exit__(self, *exc):
        from isaacgyminsertion_amd import _lib
        for k, v in self.prev.items():
            getattr(_lib.lib(), k)(v)
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


def _run(x, gy, flat, **switches):
    """forward + backward through the two ops under one setting (every switch not named: off) -> (y, grads (flat),
    workspace, profiler classes)"""
    from isaacgyminsertion_amd import _lib, ops  # noqa: F401
    B, _, H, W = x.shape
    with _mode(**{**{k: 0 for k in SWITCHES}, **switches}):
        _lib.prof_enable(True)
        try:
            y, ws = torch.ops.mi355ppo.tactile_cnn_fwd(x, flat, 32)
            g = torch.ops.mi355ppo.tactile_cnn_bwd(gy, flat, ws, H, W)
            torch.cuda.synchronize()
            classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
        finally:
            _lib.prof_enable(False)
    return y, g, ws, classes


def _inputs(B, H, W):
    gen = torch.Generator().manual_seed(1000 * B + H)
    return torch.rand(B, 3, H, W, generator=gen), torch.randn(B, 32, generator=gen)


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """one device run per shape under the mode and one with every switch off, shared by the tests below, left unchanged"""
    sd = _sd()
    x, gy = _inputs(B, H, W)
    flat = torch.cat([v.reshape(-1) for v in sd.values()]).cuda()
    y, g, ws, classes = _run(x.cuda(), gy.cuda(), flat, igi_conv_set_bf16x3=1)
    maps = _maps(ws, B, H, W)
    y0, g0, _ws0, classes0 = _run(x.cuda(), gy.cuda(), flat)
    return dict(sd=sd, x=x, gy=gy, flat=flat, y=y.cpu(), gflat=g.cpu(), g=_split(g.cpu(), sd), maps=maps,
                classes=classes, classes_off=classes0, y_off=y0.cpu(), g_off=g0.cpu())


def _conv_chunked(fn, n, chunk=128):
    return torch.cat([fn(slice(i, min(i + chunk, n))) for i in range(0, n, chunk)])


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_layerwise_forward_holds_the_fp32_bound(B, H, W):
    """a_l == relu(conv64(device a_{l-1}, W_l) + b_l), operands UN-rounded, within the project's GEMM bound per entry,
    2e-6 * (|a| (*) |W|) + 1e-6 -- the fp32 path's bound.  The bf16-rounded fp64 product of the same inputs lies outside
    that bound somewhere: what ran is not the one-plane mode."""
    c = _case(B, H, W)
    sd, maps = c["sd"], c["maps"]
    inputs = [c["x"], maps[0], maps[1]]
    for l, (kw, kb, stride) in enumerate(KEYS):
        a_in, w = inputs[l], sd[kw]
        ref = _conv_chunked(lambda s: F.relu(F.conv2d(a_in[s].double(), w.double(), sd[kb].double(), stride=stride)), B)
        bound = 2e-6 * _conv_chunked(lambda s: F.conv2d(a_in[s].abs(), w.abs(), None, stride=stride), B).double() + 1e-6
        err = (maps[l].double() - ref).abs()
        worst = float((err / bound).max())
        n = min(B, 32)
        rounded = F.relu(F.conv2d(bf16r(a_in[:n]).double(), bf16r(w).double(), sd[kb].double(), stride=stride))
        viol = float(((rounded - ref[:n]).abs() / bound[:n]).max())
        print(f"[{B}x{H}x{W}] conv{l + 1}: max err / bound = {worst:.3f} (max err {float(err.max()):.3e}); "
              f"bf16-rounded fp64 product: {viol:.1f}")
        assert worst <= 1.0, (l, worst, float(err.max()))
        assert viol > 1.0, (l, viol)


def _softargmax_linear(a3, wf, bf):
    from oracle import encoders as oe
    return F.linear(oe.spatial_softargmax(a3, True), wf, bf)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_output_from_the_device_feature_map(B, H, W):
    """y against the fp64 soft-argmax + Linear of the device's a_3: 2e-5 abs + 1e-4 rel."""
    c = _case(B, H, W)
    sd = c["sd"]
    y64 = _softargmax_linear(c["maps"][2].double(), sd["cnn.7.weight"].double(), sd["cnn.7.bias"].double())
    np.testing.assert_allclose(c["y"].numpy(), y64.numpy(), atol=2e-5, rtol=1e-4)


def _emulated_backward(c, dtype, rnd, chunk=128):
    """The backward in ``dtype`` on the CPU, from the device's activations: the soft-argmax + Linear backward from a_3
    (autograd), ReLU' from the device's maps, every convolution operand (dz_l, a_{l-1}, W_l) passed through ``rnd`` before
    each product -- the identity for this mode, bf16r for the one-plane mode; bias gradients are plain sums of dz_l.
    Chunked over the batch (additive over images)."""
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
            dzr, ar, wr = rnd(dz), rnd(ins[l]), rnd(sd[kw])
            g[kw] += conv2d_weight(ar, sd[kw].shape, dzr, stride=stride)
            g[kb] += dz.sum((0, 2, 3))
            if l > 0:
                dz = conv2d_input(ins[l].shape, wr, dzr, stride=stride) * (ins[l] > 0).to(dtype)
    return g


def _misses(c, rnd, tag):
    """the tensors whose device gradient misses |hip - emu64| <= max(3e-4 * max|g|, 3 x |emu32 - emu64|)"""
    g64 = _emulated_backward(c, torch.float64, rnd)
    g32 = _emulated_backward(c, torch.float32, rnd)
    bad = []
    for k in c["sd"]:
        ref = g64[k].numpy()
        scale = np.abs(ref).max()
        err = np.abs(c["g"][k].numpy().astype(np.float64) - ref).max()
        err32 = np.abs(g32[k].numpy().astype(np.float64) - ref).max()
        print(f"[{tag}] {k}: |hip - emu64| = {err:.3e} ({err / scale:.2e} of max|g|), |emu32 - emu64| = {err32:.3e}")
        if not err <= max(3e-4 * scale, 3.0 * err32):
            bad.append((k, err, err32, scale))
    return bad


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_gradients_match_the_unrounded_backward_and_not_the_one_plane_one(B, H, W):
    """All eight parameter tensors against the UN-rounded float64 backward from the device's activations and masks, per
    tensor within the fp32 path's bound of test_gpu_student_scale.py.  The same harness with the one-plane rounding put
    back rejects these gradients on at least one convolution weight: the check separates the two modes."""
    c = _case(B, H, W)
    bad = _misses(c, lambda t: t, f"{B}x{H}x{W} un-rounded")
    assert not bad, bad
    bad1 = _misses(c, bf16r, f"{B}x{H}x{W} one-plane")
    assert [b for b in bad1 if b[0] in ("cnn.0.weight", "cnn.2.weight", "cnn.4.weight")], bad1


def test_all_nine_products_ran_as_x3_conv_classes_at_768():
    """768 images: three tall forward tiles (conv3 with the soft-argmax partials), two position-major data gradients, three
    position-major weight gradients (conv3's on the 192-row tile), as gemm_dma_conv_x3_kernel classes with the template
    arguments of the bf16 twins -- and neither an fp32 convolution class nor a bf16-input one; with the switch off the
    launch list is the fp32 path's.  Fails without the mode."""
    c = _case(768, 32, 64)
    want = {"gemm_dma_conv_x3_kernel<32,true,true,1,2,256>": 1, "gemm_dma_conv_x3_kernel<64,true,true,1,2,256>": 1,
            "gemm_dma_conv_x3_kernel<64,true,true,6,2,256>": 1, "gemm_dma_conv_x3_kernel<64,true,true,4,2,256>": 1,
            "gemm_dma_conv_x3_kernel<32,true,true,4,2,256>": 1, "gemm_dma_conv_x3_kernel<32,false,false,5,2,256>": 1,
            "gemm_dma_conv_x3_kernel<64,false,false,5,2,256>": 1, "gemm_dma_conv_x3_kernel<64,false,false,5,2,192>": 1}
    got = {k: v for k, v in c["classes"].items() if X3_CLASS.match(k)}
    assert got == want, c["classes"]
    assert not [k for k in c["classes"] if FP32_CONV_CLASS.match(k) or BF16_CLASS.match(k)], c["classes"]
    off = c["classes_off"]
    assert not [k for k in off if X3_CLASS.match(k) or BF16_CLASS.match(k)], off
    want_off = {k.replace("gemm_dma_conv_x3_kernel", "gemm_dma_kernel"): v for k, v in want.items()}
    assert {k: v for k, v in off.items() if FP32_CONV_CLASS.match(k)} == want_off, off
    # every other launch of the two runs is the same: the mode changes no tile choice and no launch count
    strip = lambda cl: {k: v for k, v in cl.items() if not (X3_CLASS.match(k) or FP32_CONV_CLASS.match(k))}  # noqa: E731
    assert strip(c["classes"]) == strip(off)
    # the small shapes: eight x3 launches as well (128-row tiles), none booked as fp32 or bf16-input
    for shp in SHAPES[:2]:
        cl = _case(*shp)["classes"]
        assert sum(v for k, v in cl.items() if X3_CLASS.match(k)) == 8, cl
        assert not [k for k in cl if FP32_CONV_CLASS.match(k) or BF16_CLASS.match(k)], cl
        # (the fp32 path books these tiles under gemm_dma_kernel<64,...>: the totals agree)
        assert sum(cl.values()) == sum(_case(*shp)["classes_off"].values())


def _module_grads(x, gy, fwd, bwd):
    """module forward under switches ``fwd`` = (x3, bf16), backward after they were flipped to ``bwd``"""
    from isaacgyminsertion_amd import ops
    from isaacgyminsertion_amd.algo.models.transformer.tactile_cnn import CNNWithSpatialSoftArgmax
    m = CNNWithSpatialSoftArgmax(32)
    m.load_state_dict(_sd())
    m = m.cuda()
    start = ops.conv_bf16x3_enabled(), ops.conv_bf16_inputs_enabled()
    try:
        ops.conv_bf16x3(fwd[0]), ops.conv_bf16_inputs(fwd[1])
        y = m(x)
        ops.conv_bf16x3(bwd[0]), ops.conv_bf16_inputs(bwd[1])        # flipped behind the forward's back
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        assert (ops.conv_bf16x3_enabled(), ops.conv_bf16_inputs_enabled()) == (bool(bwd[0]), bool(bwd[1]))   # restored
    finally:
        ops.conv_bf16x3(start[0]), ops.conv_bf16_inputs(start[1])
    return y.detach(), [p.grad.clone() for p in m.parameters()]


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))


def test_reproducible_and_mode_is_captured_at_forward():
    """Two forward + backward runs under the mode are bit-identical (64 and 768 images); a switch flipped between forward
    and backward does not reach the backward: on/off == on/on, off/on == off/off; a forward under the one-plane mode
    followed by conv_bf16x3(True) still runs the one-plane backward -- and raises nothing, since the formula re-establishes
    BOTH recorded settings."""
    gen = torch.Generator().manual_seed(5)
    x, gy = torch.rand(64, 3, 32, 64, generator=gen).cuda(), torch.randn(64, 32, generator=gen).cuda()
    OFF, X3, BF = (False, False), (True, False), (False, True)
    on = _module_grads(x, gy, X3, X3)
    assert _same(on, _module_grads(x, gy, X3, X3))
    off = _module_grads(x, gy, OFF, OFF)
    assert not torch.equal(on[0], off[0]) and not torch.equal(on[1][0], off[1][0])
    assert _same(_module_grads(x, gy, X3, OFF), on)
    assert _same(_module_grads(x, gy, OFF, X3), off)
    bf = _module_grads(x, gy, BF, BF)
    assert not torch.equal(bf[0], on[0]) and not torch.equal(bf[0], off[0])
    assert _same(_module_grads(x, gy, BF, (True, True)), bf)
    assert _same(_module_grads(x, gy, BF, X3), bf)
    assert _same(_module_grads(x, gy, X3, BF), on)
    for shp in (SHAPES[0], SHAPES[2]):
        c = _case(*shp)
        y2, g2, _ws, _cl = _run(c["x"].cuda(), c["gy"].cuda(), c["flat"], igi_conv_set_bf16x3=1)
        assert torch.equal(y2.cpu(), c["y"]) and torch.equal(g2.cpu(), c["gflat"]), shp


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


_UNTOUCHED = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from isaacgyminsertion_amd import ops  # noqa: F401
G = np.load(%(golden)r)
tag = "tac32x64"
flat = torch.cat([torch.from_numpy(G[k]).reshape(-1) for k in G.files if k.startswith(tag + "/p/")]).cuda()
B, H, W = 64, 32, 64
gen = torch.Generator().manual_seed(1000 * B + H)
x, gy = torch.rand(B, 3, H, W, generator=gen).cuda(), torch.randn(B, 32, generator=gen).cuda()
y, ws = torch.ops.mi355ppo.tactile_cnn_fwd(x, flat, 32)
g = torch.ops.mi355ppo.tactile_cnn_bwd(gy, flat, ws, H, W)
torch.cuda.synchronize()
torch.save({"y": y.cpu(), "g": g.cpu()}, %(out)r)
"""


def test_isolation():
    """With the switch on, PointNet, ``linear``, the token encoder, ``actor_critic_infer`` and a small teacher update are
    bit-identical to switch-off.  With the switch off, the tactile forward and gradients are the bits of a process that
    never called the setter.  igi_gemm_set_bf16_inputs(1) and igi_gemm_set_bf16x3(6) alone leave them at those bits too."""
    with _mode(igi_conv_set_bf16x3=0):
        ref = _others()
    with _mode(igi_conv_set_bf16x3=1):
        got = _others()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    c = _case(64, 32, 64)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("IGI_CONV_BF16", "IGI_CONV_BF16X3", "IGI_GEMM_BF16", "IGI_GEMM_X3"):
        env.pop(k, None)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "untouched.pt")
        code = _UNTOUCHED % {"root": ROOT, "golden": os.path.join(ROOT, "tests", "golden", "encoders.npz"), "out": out}
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        child = torch.load(out)
    assert torch.equal(child["y"], c["y_off"]) and torch.equal(child["g"], c["g_off"])
    x, gy = c["x"].cuda(), c["gy"].cuda()
    for sw in ({"igi_gemm_set_bf16_inputs": 1}, {"igi_gemm_set_bf16x3": 6}):
        y1, g1, _ws, cl1 = _run(x, gy, c["flat"], **sw)
        assert torch.equal(y1.cpu(), c["y_off"]) and torch.equal(g1.cpu(), c["g_off"]), sw
        assert not [k for k in cl1 if X3_CLASS.match(k) or BF16_CLASS.match(k)], cl1


def test_both_switches_on_is_an_error():
    """igi_tactile_forward / igi_tactile_backward refuse to choose: the ops raise, and the process switches are as before."""
    from isaacgyminsertion_amd import _lib
    c = _case(64, 32, 64)
    x, gy, flat = c["x"].cuda(), c["gy"].cuda(), c["flat"]
    L = _lib.lib()
    with _mode(igi_conv_set_bf16x3=0, igi_conv_set_bf16_inputs=0):
        y, ws = torch.ops.mi355ppo.tactile_cnn_fwd(x, flat, 32)
        with _mode(igi_conv_set_bf16x3=1, igi_conv_set_bf16_inputs=1):
            with pytest.raises(RuntimeError, match="igi_tactile_forward"):
                torch.ops.mi355ppo.tactile_cnn_fwd(x, flat, 32)
            with pytest.raises(RuntimeError, match="igi_tactile_backward"):
                torch.ops.mi355ppo.tactile_cnn_bwd(gy, flat, ws, 32, 64)
            assert (L.igi_conv_set_bf16x3(-1), L.igi_conv_set_bf16_inputs(-1)) == (1, 1)
        assert (L.igi_conv_set_bf16x3(-1), L.igi_conv_set_bf16_inputs(-1)) == (0, 0)
        g = torch.ops.mi355ppo.tactile_cnn_bwd(gy, flat, ws, 32, 64)       # and the library goes on working
        torch.cuda.synchronize()
    assert torch.equal(y.cpu(), c["y_off"]) and torch.equal(g.cpu(), c["g_off"])


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
        del cfg.offline_train.model["conv_bf16x3"]
    else:
        cfg.offline_train.model.conv_bf16x3 = key
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
    before = _lib.lib().igi_conv_set_bf16x3(-1)
    _lib.prof_enable(True)
    losses, _ = agent.update()
    torch.cuda.synchronize()
    classes = {c["name"]: c["launches"] for c in _lib.prof_read()}
    _lib.prof_enable(False)
    return {"losses": [float(l) for l in losses], "classes": classes, "switch_before": before,
            "switch_after": _lib.lib().igi_conv_set_bf16x3(-1), "bf16_after": _lib.lib().igi_conv_set_bf16_inputs(-1)}

print(json.dumps({"on": run(True), "absent": run(None)}))
"""


def test_trainer_reads_the_config_key():
    """ExtrinsicAdapt (tactile + lin, 8 envs x 4 steps, 4 mini-epochs) in a child process with
    offline_train.model.conv_bf16x3=True: update() runs x3 convolution classes only, the loss falls over the update (mean
    of the last mini-epoch below the first's), and the process switch is left as it was; the same run without the key
    shows no x3 class."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("IGI_CONV_BF16", "IGI_CONV_BF16X3"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _TRAINER % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    on, absent = out["on"], out["absent"]
    assert sum(v for k, v in on["classes"].items() if X3_CLASS.match(k)) >= 8 * len(on["losses"]), on["classes"]
    assert not [k for k in on["classes"] if FP32_CONV_CLASS.match(k) or BF16_CLASS.match(k)], on["classes"]
    assert on["switch_before"] == 0 and on["switch_after"] == 0 and on["bf16_after"] == 0
    n = len(on["losses"]) // 4
    first, last = np.mean(on["losses"][:n]), np.mean(on["losses"][-n:])
    print(f"loss: first mini-epoch {first:.5f}, last {last:.5f}")
    assert np.isfinite(on["losses"]).all() and last < first, on["losses"]
    assert not [k for k in absent["classes"] if X3_CLASS.match(k) or BF16_CLASS.match(k)], absent["classes"]
    assert [k for k in absent["classes"] if FP32_CONV_CLASS.match(k)], absent["classes"]
